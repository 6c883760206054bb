// p256_sign.hip -- deterministic ECDSA-P256 signing in batches, one signature
// per lane (sign.h: RFC 6979 nonces, k*G over the width-16 G comb, no low-S).
// Three stages, split where the live state is smallest (128 B per signature
// between them, SignRec), each a plain grid of 256-thread blocks with no LDS,
// no atomics and no inter-lane waits:
//   k_sign_nonce  hash + private key -> the HMAC-DRBG's first candidate in
//                 (0, n) (at most kSignMaxCandidates), then k^-1 mod n by the
//                 constant-time divsteps.  All SHA-256, no field arithmetic.
//   k_sign_comb   R = k*G: 17 mixed additions of comb entries selected by
//                 masks, the Z == 0 test, the field inversion of Z, x mod n.
//                 No call, no scratch: a lane whose walk met (none can, sign.h)
//                 only raises a flag.
//   k_sign_tail   s = k^-1 (e + r d), the r||s row as four 16-byte stores, the
//                 ok bitmap by wave ballot, k and k^-1 overwritten with zeros.
//                 A lane flagged by the comb, or with r = 0 or s = 0, redoes
//                 its signature in sign.h's own ecdsa_sign (a real call: the
//                 exact rerun and the next candidate live there).
//   k_sign_der    r||s rows -> minimal DER in 72-byte slots plus lengths
//                 (der.h's writer), 0 where not signed.
// Private keys: a device array of 8 LE words per key and a validity word
// (register: pbftv_api.cpp).  A row whose key index is out of range or names an
// invalid key is 64 zero bytes and a 0 bit; it loads no key.
// A translation unit of its own: nothing here changes what the verify
// kernels compile to.
#include <hip/hip_runtime.h>

#include "der.h"
#include "kernels.h"
#include "sign.h"
#include "verify_kernels.h"

namespace pbftv {

namespace {

// q[0..1] k, q[2..3] k^-1, q[4] = {state, candidate index, 0, 0}, q[5..6] r
// (LE words), q[7] unused.  state: 0 no signature (bad key or no candidate),
// 1 nonce ready, 2 r ready, 3 the walk met (the tail redoes the signature).
struct alignas(128) SignRec {
  uint4 q[8];
};

constexpr uint32_t kSignNone = 0, kSignNonce = 1, kSignR = 2, kSignMet = 3;

__device__ __forceinline__ void sign_load_g(const uint4* __restrict__ gtab, int win, int idx, uint32_t ew[16]) {
  const uint4* p = gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 4;
  uint4 e[4];
  e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; e[3] = p[3];
  entry_words(e, ew);
}

__device__ __forceinline__ void store_be256(uint4* o, const uint32_t w[8]) {
  o[0] = make_uint4(bswap32(w[7]), bswap32(w[6]), bswap32(w[5]), bswap32(w[4]));
  o[1] = make_uint4(bswap32(w[3]), bswap32(w[2]), bswap32(w[1]), bswap32(w[0]));
}

// the key of row i, or "none": keys[8 j ..] = key j's words, valid[j] its flag
__device__ __forceinline__ bool sign_key(const uint32_t* __restrict__ skey_idx, uint64_t i,
                                         const uint32_t* __restrict__ keys, const uint32_t* __restrict__ valid,
                                         uint32_t nkeys, uint32_t d[8]) {
  const uint32_t j = skey_idx[i];
  if (j >= nkeys || valid[j] == 0) return false;
  const uint4 a = *reinterpret_cast<const uint4*>(keys + 8ull * j);
  const uint4 b = *reinterpret_cast<const uint4*>(keys + 8ull * j + 4);
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
  return true;
}

}  // namespace

__global__ void __launch_bounds__(256) k_sign_nonce(const uint8_t* __restrict__ hashes,
                                                    const uint32_t* __restrict__ skey_idx,
                                                    const uint32_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ valid, uint32_t nkeys, uint64_t n,
                                                    SignRec* __restrict__ rec) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t d[8], e[8], k[8], kinv[8];
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) k[j] = kinv[j] = 0;
  int cand = -1;
  if (sign_key(skey_idx, i, keys, valid, nkeys, d)) {
    load_be256(hashes + 32 * i, e);
    rfc6979_state S;
    rfc6979_init(S, d, e);
    cand = sign_nonce(S, k, 0);
    if (cand >= 0) inv_mod_n_words_ct(kinv, k);
  }
  SignRec* rp = rec + i;
  rp->q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  rp->q[1] = make_uint4(k[4], k[5], k[6], k[7]);
  rp->q[2] = make_uint4(kinv[0], kinv[1], kinv[2], kinv[3]);
  rp->q[3] = make_uint4(kinv[4], kinv[5], kinv[6], kinv[7]);
  rp->q[4] = make_uint4(cand >= 0 ? kSignNonce : kSignNone, (uint32_t)cand, 0, 0);
}

__global__ void __launch_bounds__(256) k_sign_comb(SignRec* __restrict__ rec, uint64_t n,
                                                   const uint4* __restrict__ gtab) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  SignRec* rp = rec + i;
  if (rp->q[4].x != kSignNonce) return;
  const uint4 a = rp->q[0], b = rp->q[1];
  const uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  jac R;
  const bool fin = sign_mult_fast(R, k, [&](int win, int idx, uint32_t ew[16]) { sign_load_g(gtab, win, idx, ew); });
  if (!fin || fe_is_zero(R.z)) {  // (0 < k < n: neither happens; the tail's exact form decides)
    rp->q[4].x = kSignMet;
    return;
  }
  uint32_t r[8];
  sign_r_from_point(r, R);
  rp->q[5] = make_uint4(r[0], r[1], r[2], r[3]);
  rp->q[6] = make_uint4(r[4], r[5], r[6], r[7]);
  rp->q[4].x = kSignR;
}

// The whole signature again through sign.h's ecdsa_sign: its exact rerun, its
// next candidates.  A real call that passes only addresses of global memory, so
// the tail's common path keeps its own registers.
__device__ __noinline__ bool sign_slow(const uint8_t* __restrict__ hash, const uint32_t* __restrict__ key,
                                       const uint4* __restrict__ gtab, uint4* out) {
  uint32_t e[8], d[8], r[8], s[8];
  load_be256(hash, e);
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) d[j] = key[j];
  const bool ok =
      ecdsa_sign(e, d, r, s, [&](int win, int idx, uint32_t ew[16]) { sign_load_g(gtab, win, idx, ew); });
  store_be256(out, r);
  store_be256(out + 2, s);
  return ok;
}

__global__ void __launch_bounds__(256, 2) k_sign_tail(SignRec* __restrict__ rec, const uint8_t* __restrict__ hashes,
                                                   const uint32_t* __restrict__ skey_idx,
                                                   const uint32_t* __restrict__ keys,
                                                   const uint32_t* __restrict__ valid, uint32_t nkeys, uint64_t n,
                                                   const uint4* __restrict__ gtab, uint4* __restrict__ out_rs,
                                                   uint8_t* __restrict__ okbits) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (i < n) {
    SignRec* rp = rec + i;
    const uint32_t state = rp->q[4].x;
    uint4* o = out_rs + 4 * i;
    uint32_t d[8], r[8], s[8];
    PBFTV_UNROLL for (int j = 0; j < 8; ++j) r[j] = s[j] = 0;
    bool redo = state == kSignMet;
    if (state == kSignR && sign_key(skey_idx, i, keys, valid, nkeys, d)) {
      const uint4 c = rp->q[2], dd = rp->q[3], f = rp->q[5], g = rp->q[6];
      const uint32_t kinv[8] = {c.x, c.y, c.z, c.w, dd.x, dd.y, dd.z, dd.w};
      const uint32_t rw[8] = {f.x, f.y, f.z, f.w, g.x, g.y, g.z, g.w};
      uint32_t e[8], sw[8];
      load_be256(hashes + 32 * i, e);
      const bool s_ok = sign_s(sw, e, d, rw, kinv);
      ok = s_ok && !words_is_zero(rw);
      redo = !ok;
      if (ok) {
        PBFTV_UNROLL for (int j = 0; j < 8; ++j) {
          r[j] = rw[j];
          s[j] = sw[j];
        }
      }
    }
    const uint4 z = make_uint4(0, 0, 0, 0);
    rp->q[0] = z; rp->q[1] = z; rp->q[2] = z; rp->q[3] = z;  // k and k^-1 do not outlive the batch
    if (redo) {
      ok = sign_slow(hashes + 32 * i, keys + 8ull * skey_idx[i], gtab, o);
    } else {
      store_be256(o, r);
      store_be256(o + 2, s);
    }
  }
  if (okbits != nullptr) {  // (uniform) LSB-first bitmap by wave ballot, lanes 0..7 store one byte each
    const unsigned long long m = __ballot(ok);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave_base = i - lane;
    if (lane < 8 && wave_base + 8 * lane < n) okbits[(wave_base >> 3) + lane] = (uint8_t)(m >> (8 * lane));
  }
}

// slot i = out + 72 i (8-byte aligned: 72 = 9 x 8)
__global__ void __launch_bounds__(256) k_sign_der(const uint8_t* __restrict__ rs, const uint8_t* __restrict__ okbits,
                                                  uint64_t n, uint8_t* __restrict__ out, uint32_t* __restrict__ out_len) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint8_t* slot = out + 72 * i;
  uint32_t len = 0;
  if ((okbits[i >> 3] >> (i & 7)) & 1u) {
    len = der_from_rs(rs + 64 * i, slot);
  } else {
    uint2* s2 = reinterpret_cast<uint2*>(slot);
    PBFTV_UNROLL for (int j = 0; j < 9; ++j) s2[j] = make_uint2(0, 0);
  }
  out_len[i] = len;
}

size_t sign_record_bytes(uint64_t n) { return (size_t)n * sizeof(SignRec); }

bool sign_key_valid(const uint8_t be[32]) {
  uint32_t d[8];
  sign_words_from_be(d, be);
  return sign_scalar_ok(d);
}

void sign_key_words(const uint8_t be[32], uint32_t out[8]) { sign_words_from_be(out, be); }

hipError_t launch_sign_stage(int stage, const SignArgs& a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  if (a.n >> 32) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
  SignRec* rec = reinterpret_cast<SignRec*>(a.rec);
  const uint4* gtab = reinterpret_cast<const uint4*>(a.gtab);
  switch (stage) {
    case kSignStageNonce:
      hipLaunchKernelGGL(k_sign_nonce, grid, block, 0, st, a.hashes, a.skey_idx, a.keys, a.key_valid, a.nkeys, a.n, rec);
      break;
    case kSignStageComb:
      hipLaunchKernelGGL(k_sign_comb, grid, block, 0, st, rec, a.n, gtab);
      break;
    case kSignStageTail:
      hipLaunchKernelGGL(k_sign_tail, grid, block, 0, st, rec, a.hashes, a.skey_idx, a.keys, a.key_valid, a.nkeys, a.n,
                         gtab, reinterpret_cast<uint4*>(a.out_rs), a.okbits);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_sign_der(const uint8_t* rs, const uint8_t* okbits, uint64_t n, uint8_t* out_der, uint32_t* out_len,
                           hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n >> 32) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_sign_der, grid, block, 0, st, rs, okbits, n, out_der, out_len);
  return hipGetLastError();
}

}  // namespace pbftv
