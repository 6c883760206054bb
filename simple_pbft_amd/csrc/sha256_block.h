// sha256_block.h -- the SHA-256 compression function for code that g++ and
// hipcc both compile (sign.h's HMAC-DRBG).  On the device the rotates are
// v_alignbit_b32 and Maj and the three-way XORs are v_bitop3_b32, the forms
// of sha256_kernels.hip's compress; on the host it is plain C++.  That file
// keeps its own copy: the message kernels are not recompiled through this
// header.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PBFTV_SHA_HD __host__ __device__ __forceinline__
#define PBFTV_SHA_UNROLL _Pragma("unroll")
#else
#define PBFTV_SHA_HD static inline
#define PBFTV_SHA_UNROLL
#endif

namespace pbftv {

static constexpr uint32_t kSha256Iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

static constexpr uint32_t kSha256K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
#else
static inline uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static inline uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
static inline uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }
#endif

// st <- compress(st, block): w holds the block's 16 big-endian words and is
// used as the message schedule's ring (overwritten).
PBFTV_SHA_HD void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  PBFTV_SHA_UNROLL for (int r = 0; r < 64; ++r) {
    uint32_t wr;
    if (r < 16) {
      wr = w[r];
    } else {
      const uint32_t x = w[(r + 1) & 15], y = w[(r + 14) & 15];
      const uint32_t s0 = sha_xor3(sha_rotr(x, 7), sha_rotr(x, 18), x >> 3);
      const uint32_t s1 = sha_xor3(sha_rotr(y, 17), sha_rotr(y, 19), y >> 10);
      w[r & 15] += s0 + w[(r + 9) & 15] + s1;
      wr = w[r & 15];
    }
    const uint32_t S1 = sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25));
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + kSha256K[r] + wr;
    const uint32_t S0 = sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22));
    const uint32_t t2 = S0 + sha_maj(a, b, c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

}  // namespace pbftv
