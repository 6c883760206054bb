// p256_varbase.hip -- ECDSA-P256 batch verification under keys that were never
// registered: every signature carries its own public key (varbase.h).
//   k_varbase_keys  key_check per signature: validity word, identity index
//                   (so the unchanged stage 1, k_ecdsa_scalars, treats lane i's
//                   key as "key i of n"), the key left in Montgomery form.
//   k_varbase_keys_sec1<FMT>  the same for keys in SEC1 wire form (sec1.h:
//                   33 B compressed -- a square root mod p per key -- or 65 B
//                   uncompressed), staged through LDS because a 33- or 65-byte
//                   stride is not word aligned.
//   k_varbase       one signature per lane, grid-stride: the lane's table
//                   1Q .. 8Q in global scratch, the 4-bit fixed-window ladder
//                   for u2*Q, 17 mixed additions of the width-16 G comb for
//                   u1*G, ecdsa_check, bitmap by wave ballot.
// A translation unit of its own: nothing here changes what the registered
// path's kernels compile to.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "sec1.h"
#include "varbase.h"
#include "verify_kernels.h"

namespace pbftv {

constexpr int kVbBlock = 256;
#ifndef PBFTV_VARBASE_WAVES
// min waves per SIMD of k_varbase.  2: 256 VGPRs; the ~70 spilled registers
// are all outside the ladder and G-part loops (the round's set-up, the table
// build, around the call of the exact rerun).  1 (256 VGPRs + ~100 AGPRs, no
// spill at all) measured 22.2 ms per 1M against 19.7 ms.
#define PBFTV_VARBASE_WAVES 2
#endif
constexpr int kVbBlocksPerCu = PBFTV_VARBASE_WAVES;  // 4 waves per block, 4 SIMDs per CU
constexpr int kVbKeyWords = 18;                      // x, y: 9 limbs each

// keys[w * n + i]: limb w of signature i's key (x limbs 0..8, y limbs 9..17)
__global__ void __launch_bounds__(256) k_varbase_keys(const uint8_t* __restrict__ pub_xy, uint64_t n,
                                                      uint32_t* __restrict__ valid, uint32_t* __restrict__ idx,
                                                      uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t xw[8], yw[8];
  load_be256(pub_xy + 64 * i, xw);
  load_be256(pub_xy + 64 * i + 32, yw);
  fe xm, ym;
  const bool ok = key_check(xw, yw, xm, ym);
  if (!ok) {  // a harmless point (never used: valid = 0 makes stage 1 reject the signature)
    fe_set(xm, kGxMont);
    fe_set(ym, kGyMont);
  }
  valid[i] = ok ? 1u : 0u;
  idx[i] = (uint32_t)i;
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) {
    keys[(uint64_t)l * n + i] = xm.v[l];
    keys[(uint64_t)(9 + l) * n + i] = ym.v[l];
  }
}

// Keys in SEC1 wire form, one per lane, same outputs as k_varbase_keys.  A
// block's 256 keys are one contiguous span that starts on a word boundary
// (256 * stride is a multiple of 4 and the column is 16-B aligned): the block
// copies it to LDS with coalesced word loads -- the ragged tail of the column's
// last word byte by byte, so nothing past the last key is read -- and each
// lane decodes its key from there.
template <int FMT>
__global__ void __launch_bounds__(256) k_varbase_keys_sec1(const uint8_t* __restrict__ wire, uint64_t n,
                                                           uint32_t* __restrict__ valid, uint32_t* __restrict__ idx,
                                                           uint32_t* __restrict__ keys) {
  static_assert(FMT == kKeySec1Compressed || FMT == kKeySec1Uncompressed, "a SEC1 format");
  constexpr uint32_t kStride = FMT == kKeySec1Compressed ? 33 : 65;
  __shared__ uint32_t stage[kStride * 256 / 4];
  const uint64_t first = (uint64_t)blockIdx.x * 256;  // (< n: the grid is ceil(n / 256) blocks)
  const uint32_t cnt = (uint32_t)(n - first < 256 ? n - first : 256);
  const uint32_t bytes = cnt * kStride;
  const uint8_t* src = wire + first * kStride;
  for (uint32_t w = threadIdx.x; 4 * w < bytes; w += 256) {
    uint32_t v = 0;
    if (4 * w + 4 <= bytes) {
      v = *reinterpret_cast<const uint32_t*>(src + 4 * w);
    } else {
      for (uint32_t k = 0; 4 * w + k < bytes; ++k) v |= (uint32_t)src[4 * w + k] << (8 * k);
    }
    stage[w] = v;
  }
  __syncthreads();
  if (threadIdx.x >= cnt) return;
  const uint64_t i = first + threadIdx.x;
  fe xm, ym;
  const bool ok = sec1_key_check(reinterpret_cast<const uint8_t*>(stage) + threadIdx.x * kStride, FMT, xm, ym);
  if (!ok) {  // (as k_varbase_keys: G stands in, valid = 0 rejects the signature)
    fe_set(xm, kGxMont);
    fe_set(ym, kGyMont);
  }
  valid[i] = ok ? 1u : 0u;
  idx[i] = (uint32_t)i;
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) {
    keys[(uint64_t)l * n + i] = xm.v[l];
    keys[(uint64_t)(9 + l) * n + i] = ym.v[l];
  }
}

// The lane's table in the global scratch: limb w of entry k at
// tab[(k * 27 + w) * L + slot] -- [entry][word][lane], so the lanes of a wave
// that read the same entry read consecutive words.
struct VbTab {
  uint32_t* p;  // tab + slot
  uint64_t L;
  __device__ __forceinline__ void store(int k, const jac& q) const {
    uint32_t* e = p + (uint64_t)k * kVbPointWords * L;
    PBFTV_UNROLL for (int l = 0; l < 9; ++l) {
      e[(uint64_t)l * L] = q.x.v[l];
      e[(uint64_t)(9 + l) * L] = q.y.v[l];
      e[(uint64_t)(18 + l) * L] = q.z.v[l];
    }
  }
  __device__ __forceinline__ void load(int k, jac& q) const {
    const uint32_t* e = p + (uint64_t)k * kVbPointWords * L;
    PBFTV_UNROLL for (int l = 0; l < 9; ++l) {
      q.x.v[l] = e[(uint64_t)l * L];
      q.y.v[l] = e[(uint64_t)(9 + l) * L];
      q.z.v[l] = e[(uint64_t)(18 + l) * L];
    }
  }
};

__device__ __forceinline__ void vb_load_g(const uint4* __restrict__ gtab, int win, int idx, uint32_t ew[16]) {
  const uint4* p = gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 4;
  uint4 e[4];
  e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; e[3] = p[3];
  entry_words(e, ew);
}

// The exact rerun is a real call, so its registers do not inflate the fast
// path's allocation; it re-reads its inputs and the lane's table from memory
// and returns only the accept bit (comb2_checked_verify's pattern).
__device__ __noinline__ bool vb_checked_verify(const SigRec* __restrict__ rp, uint32_t* tab_lane, uint64_t L,
                                               const uint4* __restrict__ gtab) {
  const uint4 a = rp->q[0], b = rp->q[1], c = rp->q[2], dd = rp->q[3], e = rp->q[4], f = rp->q[5];
  const uint32_t u1[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const uint32_t u2[8] = {c.x, c.y, c.z, c.w, dd.x, dd.y, dd.z, dd.w};
  const uint32_t r[8] = {e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w};
  const VbTab T{tab_lane, L};
  jac R;
  const bool fin = varbase_mult_exact(
      R, u1, u2, [&](int k, jac& q) { T.load(k, q); },
      [&](int win, int idx, uint32_t ew[16]) { vb_load_g(gtab, win, idx, ew); });
  return ecdsa_check(R, fin, r);
}

__global__ void __launch_bounds__(kVbBlock, PBFTV_VARBASE_WAVES)
    k_varbase(const SigRec* __restrict__ rec, const uint32_t* __restrict__ keys, uint64_t n,
              const uint4* __restrict__ gtab, uint32_t* tab, uint8_t* __restrict__ bitmap) {
  const uint32_t t = threadIdx.x;
  const uint64_t L = (uint64_t)gridDim.x * kVbBlock;
  const VbTab T{tab + (uint64_t)blockIdx.x * kVbBlock + t, L};
  // rounds of L signatures; the bound is block-uniform, so whole waves stay
  // together for the ballot
  for (uint64_t base = (uint64_t)blockIdx.x * kVbBlock; base < n; base += L) {
    const uint64_t p = base + t;
    const SigRec* rp = rec + p;
    uint4 meta = make_uint4(0, 0, 0, 0);
    if (p < n) meta = rp->q[6];
    // a lane without a valid signature runs the same steps on u1 = u2 = 0
    // (every digit zero: it adds nothing) with G as its key
    const bool act = meta.z != 0;
    fe x, y;
    fe_set(x, kGxMont);
    fe_set(y, kGyMont);
    uint4 a = make_uint4(0, 0, 0, 0), b = a, c = a, dd = a;
    if (act) {
      PBFTV_UNROLL for (int l = 0; l < 9; ++l) {
        x.v[l] = keys[(uint64_t)l * n + p];
        y.v[l] = keys[(uint64_t)(9 + l) * n + p];
      }
      a = rp->q[0];
      b = rp->q[1];
      c = rp->q[2];
      dd = rp->q[3];
    }
    const uint32_t u1[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t u2[8] = {c.x, c.y, c.z, c.w, dd.x, dd.y, dd.z, dd.w};
    vb_build_table(x, y, [&](int k, const jac& q) { T.store(k, q); });
    jac R;
    const int fin = varbase_mult_fast(
        R, u1, u2, [&](int k, jac& q) { T.load(k, q); },
        [&](int win, int idx, uint32_t ew[16]) { vb_load_g(gtab, win, idx, ew); });
    bool ok = false;
    if (act) {
      if (fin < 0) {
        ok = vb_checked_verify(rp, T.p, L, gtab);
      } else {
        const uint4 e = rp->q[4], f = rp->q[5];
        const uint32_t r[8] = {e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w};
        ok = ecdsa_check(R, fin == 1, r);
      }
    }
    // arrival order: LSB-first bitmap by wave ballot, lanes 0..7 store one byte each
    const unsigned long long m = __ballot(ok);
    const uint32_t lane = t & 63u;
    const uint64_t wave_base = p - lane;
    if (lane < 8 && wave_base + 8 * lane < n) bitmap[(wave_base >> 3) + lane] = (uint8_t)(m >> (8 * lane));
  }
}

size_t varbase_aux_bytes(uint64_t n) { return (size_t)n * (2 + kVbKeyWords) * 4; }

uint64_t varbase_lanes(int cus) {
  uint64_t lanes = (uint64_t)std::max(cus, 1) * kVbBlocksPerCu * kVbBlock;
  if (const char* e = getenv("PBFTV_VARBASE_LANES")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v > 0) lanes = std::min<uint64_t>(v, 1ull << 24);
  }
  return (lanes + kVbBlock - 1) / kVbBlock * kVbBlock;
}

size_t varbase_table_bytes(uint64_t lanes) { return (size_t)lanes * kVbLaneWords * 4; }

static_assert(kVarbaseKeyXY == kKeyXY && kVarbaseKeySec1Compressed == kKeySec1Compressed &&
                  kVarbaseKeySec1Uncompressed == kKeySec1Uncompressed,
              "kernels.h and sec1.h name the key formats alike");

uint32_t varbase_key_bytes(int key_format) { return sec1_key_bytes(key_format); }

hipError_t launch_varbase_keys(const uint8_t* keys, int key_format, uint64_t n, void* aux, hipStream_t st) {
  if (n == 0) return hipSuccess;
  uint32_t* w = reinterpret_cast<uint32_t*>(aux);
  const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
  if (key_format == kKeyXY) {
    hipLaunchKernelGGL(k_varbase_keys, grid, block, 0, st, keys, n, w, w + n, w + 2 * n);
  } else if ((uintptr_t)keys & 3u) {  // the SEC1 kernels load the column by words
    return hipErrorInvalidValue;
  } else if (key_format == kKeySec1Compressed) {
    hipLaunchKernelGGL(k_varbase_keys_sec1<kKeySec1Compressed>, grid, block, 0, st, keys, n, w, w + n, w + 2 * n);
  } else if (key_format == kKeySec1Uncompressed) {
    hipLaunchKernelGGL(k_varbase_keys_sec1<kKeySec1Uncompressed>, grid, block, 0, st, keys, n, w, w + n, w + 2 * n);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

const uint32_t* varbase_valid(const void* aux, uint64_t) { return reinterpret_cast<const uint32_t*>(aux); }
const uint32_t* varbase_index(const void* aux, uint64_t n) { return reinterpret_cast<const uint32_t*>(aux) + n; }

hipError_t launch_varbase(const void* rec, const void* aux, uint64_t n, const uint32_t* gtab, void* tab,
                          uint64_t lanes, uint8_t* bitmap, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (lanes == 0 || lanes % kVbBlock) return hipErrorInvalidValue;
  const uint64_t blocks = std::min<uint64_t>((n + kVbBlock - 1) / kVbBlock, lanes / kVbBlock);
  hipLaunchKernelGGL(k_varbase, dim3((uint32_t)blocks), dim3(kVbBlock), 0, st, reinterpret_cast<const SigRec*>(rec),
                     reinterpret_cast<const uint32_t*>(aux) + 2 * n, n, reinterpret_cast<const uint4*>(gtab),
                     reinterpret_cast<uint32_t*>(tab), bitmap);
  return hipGetLastError();
}

}  // namespace pbftv
