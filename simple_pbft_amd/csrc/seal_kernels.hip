// seal_kernels.hip -- what a replica posts, built on the device: the signed
// wire form of votes, replies and pre-prepares (gojson_enc.h's *_signed
// encoders) packed back to back into one blob.
//
// After the encoder, k_sha256 and the signer have run, three steps remain:
//   lengths  one lane per message: wire.h's arithmetic on the preimage length
//            the encoder wrote and the signature lengths; 0 for an unsigned row
//   offsets  the exclusive scan of the lengths into 64-bit offsets and the
//            total, as three plain launches -- per-block sums, one workgroup
//            that scans the sums with a running carry, per-block offsets.  No
//            workgroup waits on another, no atomics, no flags.
//   write    one lane per message runs the *_signed encoder into blob + off[i]
// The sink of the write is bounded by the message's own length: a byte past it
// goes to the dump bytes behind the blob, never into a neighbour.
#include <hip/hip_runtime.h>

#include "gojson_enc.h"
#include "kernels.h"
#include "wire.h"

namespace pbftv {

namespace {

constexpr uint32_t kT = wire::kScanBlock;
static_assert(wire::kScanBlock == 256 && wire::kScanChunk == 256, "the scans below are written for 256 lanes");

// byte sink into the message's own bytes of the blob: [p, p + cap); what would
// land past them lands in dump (kSealDumpBytes, shared, never read)
struct BoundedSink {
  uint8_t* p;
  uint32_t n, cap;
  uint8_t* dump;
  __device__ void put(uint8_t b) {
    if (n < cap) p[n] = b;
    ++n;
  }
  __device__ uint8_t* grow(uint32_t k) {  // k <= 21 (gojson_enc.h put_int)
    uint8_t* r = n + k <= cap ? p + n : dump;
    n += k;
    return r;
  }
};

__device__ __forceinline__ const uint8_t* str(const StrCol& c, uint64_t i) { return c.data + c.off[i]; }

__device__ __forceinline__ bool ok_bit(const uint8_t* okbits, uint64_t i) { return (okbits[i >> 3] >> (i & 7)) & 1u; }

__device__ __forceinline__ gojson::SigField sig_of(const SealSigs& s, uint64_t i) {
  return gojson::SigField{s.sig + (uint64_t)s.stride * i, s.len ? s.len[i] : wire::kSigRsLen, false};
}

// exclusive scan of one value per lane over the 256 lanes of the workgroup;
// *sum = the workgroup's total.  Every lane calls it.
__device__ uint64_t block_scan(uint64_t v, uint64_t* lds, uint64_t* sum) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kT; d <<= 1) {
    const uint64_t a = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += a;
    __syncthreads();
  }
  const uint64_t incl = lds[t];
  *sum = lds[kT - 1];
  __syncthreads();  // (lds is free for the next call)
  return incl - v;
}

}  // namespace

// has_req == nullptr: votes and replies
__global__ void __launch_bounds__(256) k_seal_lengths(const uint32_t* __restrict__ pre_len, SealSigs s,
                                                      const uint8_t* __restrict__ has_req, SealReqSigs rq, uint64_t n,
                                                      uint32_t* __restrict__ out_len) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t w = 0;
  if (ok_bit(s.okbits, i)) {
    const uint32_t sl = s.len ? s.len[i] : wire::kSigRsLen;
    if (has_req) {
      const bool has = has_req[i] != 0;
      w = wire::preprepare_signed_len(pre_len[i], has, has ? rq.col.len[i] : 0, has ? rq.nil[i] != 0 : true, sl);
    } else {
      w = wire::signed_len(pre_len[i], sl);
    }
  }
  out_len[i] = (uint32_t)w;
}

__global__ void __launch_bounds__(256) k_seal_block_sums(const uint32_t* __restrict__ len, uint64_t n,
                                                         uint64_t* __restrict__ bsum) {
  __shared__ uint64_t lds[kT];
  const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
  uint64_t sum;
  (void)block_scan(i < n ? len[i] : 0, lds, &sum);
  if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// one workgroup: bsum[0 .. nb) -> its exclusive prefix sums in place, *total
__global__ void __launch_bounds__(256) k_seal_scan_sums(uint64_t* __restrict__ bsum, uint64_t nb,
                                                        uint64_t* __restrict__ total) {
  __shared__ uint64_t lds[kT];
  uint64_t carry = 0;
  for (uint64_t base = 0; base < nb; base += wire::kScanChunk) {
    const uint64_t j = base + threadIdx.x;
    uint64_t sum;
    const uint64_t ex = block_scan(j < nb ? bsum[j] : 0, lds, &sum);
    if (j < nb) bsum[j] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(256) k_seal_offsets(const uint32_t* __restrict__ len, uint64_t n,
                                                      const uint64_t* __restrict__ bsum, uint64_t* __restrict__ off) {
  __shared__ uint64_t lds[kT];
  const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
  uint64_t sum;
  const uint64_t ex = block_scan(i < n ? len[i] : 0, lds, &sum);
  if (i < n) off[i] = bsum[blockIdx.x] + ex;
}

__global__ void __launch_bounds__(256) k_seal_votes(VoteCols c, SealSigs s, uint64_t n,
                                                    const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                    uint8_t* __restrict__ blob, uint8_t* __restrict__ dump) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || len[i] == 0) return;
  BoundedSink o{blob + off[i], 0, len[i], dump};
  const gojson::SigField sg = sig_of(s, i);
  gojson::vote_signed(o, c.view[i], c.seq[i], str(c.digest, i), c.digest.len[i], str(c.node, i), c.node.len[i],
                      c.type[i], sg.p, sg.n, false);
}

__global__ void __launch_bounds__(256) k_seal_replies(ReplyCols c, SealSigs s, uint64_t n,
                                                      const uint64_t* __restrict__ off,
                                                      const uint32_t* __restrict__ len, uint8_t* __restrict__ blob,
                                                      uint8_t* __restrict__ dump) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || len[i] == 0) return;
  BoundedSink o{blob + off[i], 0, len[i], dump};
  gojson::reply_signed(o, c.view[i], c.ts[i], str(c.cid, i), c.cid.len[i], str(c.node, i), c.node.len[i],
                       str(c.result, i), c.result.len[i], sig_of(s, i));
}

__global__ void __launch_bounds__(256) k_seal_preprepares(PrePrepareCols c, SealSigs s, SealReqSigs rq, uint64_t n,
                                                          const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ len,
                                                          uint8_t* __restrict__ blob, uint8_t* __restrict__ dump) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || len[i] == 0) return;
  BoundedSink o{blob + off[i], 0, len[i], dump};
  const bool has = c.has_req[i] != 0;
  const bool rnil = has ? rq.nil[i] != 0 : true;
  const uint32_t rn = rnil ? 0 : rq.col.len[i];
  const gojson::SigField rs{rn ? str(rq.col, i) : nullptr, rn, rnil};
  gojson::preprepare_signed(o, c.view[i], c.seq[i], str(c.digest, i), c.digest.len[i], has, has ? c.req.ts[i] : 0,
                            str(c.req.cid, i), has ? c.req.cid.len[i] : 0, str(c.req.op, i),
                            has ? c.req.op.len[i] : 0, has ? c.req.seq[i] : 0, rs, sig_of(s, i));
}

static inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

hipError_t launch_seal_lengths(const uint32_t* pre_len, const SealSigs& s, const uint8_t* has_req,
                               const SealReqSigs& rq, uint64_t n, uint32_t* out_len, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seal_lengths, grid_for(n), dim3(256), 0, st, pre_len, s, has_req, rq, n, out_len);
  return hipGetLastError();
}

size_t seal_scan_scratch_bytes(uint64_t n) { return 8 * ((n + kT - 1) / kT) + 8; }

hipError_t launch_seal_offsets(const uint32_t* len, uint64_t n, void* scratch, uint64_t* off, uint64_t* total,
                               hipStream_t st) {
  if (n == 0) return hipSuccess;
  uint64_t* bsum = static_cast<uint64_t*>(scratch);
  const uint64_t nb = (n + kT - 1) / kT;
  hipLaunchKernelGGL(k_seal_block_sums, grid_for(n), dim3(256), 0, st, len, n, bsum);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_seal_scan_sums, dim3(1), dim3(256), 0, st, bsum, nb, total);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_seal_offsets, grid_for(n), dim3(256), 0, st, len, n, bsum, off);
  return hipGetLastError();
}

hipError_t launch_seal_votes(const VoteCols& c, const SealSigs& s, uint64_t n, const uint64_t* off,
                             const uint32_t* len, uint8_t* blob, uint8_t* dump, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seal_votes, grid_for(n), dim3(256), 0, st, c, s, n, off, len, blob, dump);
  return hipGetLastError();
}

hipError_t launch_seal_replies(const ReplyCols& c, const SealSigs& s, uint64_t n, const uint64_t* off,
                               const uint32_t* len, uint8_t* blob, uint8_t* dump, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seal_replies, grid_for(n), dim3(256), 0, st, c, s, n, off, len, blob, dump);
  return hipGetLastError();
}

hipError_t launch_seal_preprepares(const PrePrepareCols& c, const SealSigs& s, const SealReqSigs& rq, uint64_t n,
                                   const uint64_t* off, const uint32_t* len, uint8_t* blob, uint8_t* dump,
                                   hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seal_preprepares, grid_for(n), dim3(256), 0, st, c, s, rq, n, off, len, blob, dump);
  return hipGetLastError();
}

}  // namespace pbftv
