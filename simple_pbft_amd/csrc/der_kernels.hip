// der_kernels.hip -- ASN.1 DER ECDSA signatures normalised to r||s on the
// device (der.h: go1.19 crypto/ecdsa.VerifyASN1's parse, the same code the
// host runs).
//   k_der_to_rs  one signature per lane: the encoding's header bytes and its
//                two integers are fetched at computed addresses as 4-byte-
//                aligned dwords, each of which holds at least one of the first
//                min(len, 72) bytes of the encoding -- nothing before, between
//                or after the encodings is needed, whatever order they lie in
//                and whatever lengths[i] claims (der.h: no parsed encoding is
//                longer than 72 bytes).  The offset of an encoding of length 0
//                is not read.  r||s leaves as four 16-byte stores per lane
//                (zeros when not parsed), the optional LSB-first `parsed`
//                bitmap by wave ballot.  No LDS, no scratch: every register
//                array is indexed by unrolled loops only.
// A translation unit of its own: nothing here changes what the verify
// kernels compile to.
#include <hip/hip_runtime.h>

#include "der.h"
#include "kernels.h"

namespace pbftv {

namespace {

// der.h's dword reader over global memory: base = the encoding's address
// rounded down to a dword
struct GlobalDwords {
  const uint8_t* base;
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
    return *reinterpret_cast<const uint32_t*>(base + 4 * (uint64_t)k);
  }
};

}  // namespace

__global__ void __launch_bounds__(256) k_der_to_rs(const uint8_t* __restrict__ data,
                                                   const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lengths, uint64_t n,
                                                   uint4* __restrict__ out_rs, uint8_t* __restrict__ parsed) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (i < n) {
    uint32_t rs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) rs[k] = 0;
    const uint32_t len = lengths[i];
    if (len != 0) {
      const uint64_t addr = reinterpret_cast<uint64_t>(data) + offsets[i];
      const DerDwordReader<GlobalDwords> rd{{reinterpret_cast<const uint8_t*>(addr & ~(uint64_t)3)},
                                            (uint32_t)addr & 3u};
      ok = der_to_rs_words(rd, len, rs);
    }
    uint4* o = out_rs + 4 * i;
    o[0] = make_uint4(rs[0], rs[1], rs[2], rs[3]);
    o[1] = make_uint4(rs[4], rs[5], rs[6], rs[7]);
    o[2] = make_uint4(rs[8], rs[9], rs[10], rs[11]);
    o[3] = make_uint4(rs[12], rs[13], rs[14], rs[15]);
  }
  if (parsed != nullptr) {  // (uniform) LSB-first bitmap by wave ballot, lanes 0..7 store one byte each
    const unsigned long long m = __ballot(ok);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave_base = i - lane;
    if (lane < 8 && wave_base + 8 * lane < n) parsed[(wave_base >> 3) + lane] = (uint8_t)(m >> (8 * lane));
  }
}

hipError_t launch_der_to_rs(const uint8_t* data, const uint64_t* offsets, const uint32_t* lengths, uint64_t n,
                            uint8_t* out_rs, uint8_t* parsed, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n >> 32) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_der_to_rs, grid, block, 0, st, data, offsets, lengths, n, reinterpret_cast<uint4*>(out_rs),
                     parsed);
  return hipGetLastError();
}

}  // namespace pbftv
