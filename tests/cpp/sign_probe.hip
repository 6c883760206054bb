// sign_probe.hip -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_sign_probe.py).
//
// sign.h as hipcc compiles it for gfx950, one lane per case: the RFC 6979
// DRBG's first three candidates, and ecdsa_sign_with_k under a nonce the test
// chooses -- the library exports no sign-with-k, so this is where the comb
// walk's digit seams reach the device code.  Built to tests/cpp/libsign_probe.so
// with the product library's flags; it does not link libpbftv.so and the
// product never loads it.
//
// Every entry point takes host arrays (32 big-endian bytes per value) and a
// case count, allocates, copies, launches, synchronises and frees on its own,
// and returns the hipError_t (-1: an argument out of range).  sp_set_g_table
// uploads the width-16 comb table of G once (the CPU harness builds it);
// sp_release frees it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../simple_pbft_amd/csrc/sign.h"
#include "../../simple_pbft_amd/csrc/verify_kernels.h"

using namespace pbftv;

namespace {

uint4* g_gtab = nullptr;

__device__ __forceinline__ void probe_load_g(const uint4* __restrict__ gtab, int win, int idx, uint32_t ew[16]) {
  const uint4* p = gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 4;
  uint4 e[4];
  e[0] = p[0]; e[1] = p[1]; e[2] = p[2]; e[3] = p[3];
  entry_words(e, ew);
}

__device__ __forceinline__ void probe_store_be(uint8_t* out, const uint32_t w[8]) {
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) o[j] = bswap32(w[7 - j]);
}

// in: d, h1 (n x 32 B each); out: n x 3 x 32 B
__global__ __launch_bounds__(64) void k_probe_drbg(const uint8_t* d_be, const uint8_t* h_be, uint8_t* out, int n) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= n) return;
  uint32_t d[8], h[8], k[8];
  load_be256(d_be + 32 * (size_t)i, d);
  load_be256(h_be + 32 * (size_t)i, h);
  rfc6979_state S;
  rfc6979_init(S, d, h);
  PBFTV_NOUNROLL for (int j = 0; j < 3; ++j) {
    rfc6979_next(S, k);
    probe_store_be(out + 96 * (size_t)i + 32 * j, k);
  }
}

// in: e, d, k (n x 32 B each); out: r||s (n x 64 B, zeros where refused), ok and path words
__global__ __launch_bounds__(64) void k_probe_sign_with_k(const uint8_t* e_be, const uint8_t* d_be,
                                                          const uint8_t* k_be, const uint4* gtab, uint8_t* out_rs,
                                                          uint32_t* out_ok, uint32_t* out_path, int n) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= n) return;
  uint32_t e[8], d[8], k[8], r[8], s[8];
  load_be256(e_be + 32 * (size_t)i, e);
  load_be256(d_be + 32 * (size_t)i, d);
  load_be256(k_be + 32 * (size_t)i, k);
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) r[j] = s[j] = 0;
  int path = 0;
  const bool ok = ecdsa_sign_with_k(
      e, d, k, r, s, [&](int win, int idx, uint32_t ew[16]) { probe_load_g(gtab, win, idx, ew); }, &path);
  probe_store_be(out_rs + 64 * (size_t)i, r);
  probe_store_be(out_rs + 64 * (size_t)i + 32, s);
  out_ok[i] = ok ? 1u : 0u;
  out_path[i] = (uint32_t)path;
}

struct Bufs {
  void* p[8] = {};
  int n = 0;
  hipError_t alloc(void** out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess) p[n++] = *out;
    return e;
  }
  ~Bufs() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
};

}  // namespace

extern "C" {

uint64_t sp_g_table_bytes() { return CombGeom<kVbGBits>::kBytes; }

int sp_set_g_table(const uint32_t* table) {
  if (!table) return -1;
  hipError_t e = hipSuccess;
  if (!g_gtab) e = hipMalloc(&g_gtab, CombGeom<kVbGBits>::kBytes);
  if (e == hipSuccess) e = hipMemcpy(g_gtab, table, CombGeom<kVbGBits>::kBytes, hipMemcpyHostToDevice);
  return (int)e;
}

void sp_release() {
  if (g_gtab) (void)hipFree(g_gtab);
  g_gtab = nullptr;
}

int sp_drbg(const uint8_t* d_be, const uint8_t* h_be, uint8_t* out, int n) {
  if (n <= 0 || !d_be || !h_be || !out) return -1;
  Bufs b;
  uint8_t *dd = nullptr, *dh = nullptr, *dout = nullptr;
  hipError_t e = b.alloc((void**)&dd, 32 * (size_t)n);
  if (e == hipSuccess) e = b.alloc((void**)&dh, 32 * (size_t)n);
  if (e == hipSuccess) e = b.alloc((void**)&dout, 96 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(dd, d_be, 32 * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dh, h_be, 32 * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, 96 * (size_t)n);
  if (e == hipSuccess) {
    k_probe_drbg<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(dd, dh, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, 96 * (size_t)n, hipMemcpyDeviceToHost);
  return (int)e;
}

int sp_sign_with_k(const uint8_t* e_be, const uint8_t* d_be, const uint8_t* k_be, uint8_t* out_rs, uint32_t* out_ok,
                   uint32_t* out_path, int n) {
  if (n <= 0 || !e_be || !d_be || !k_be || !out_rs || !out_ok || !out_path || !g_gtab) return -1;
  Bufs b;
  uint8_t *de = nullptr, *dd = nullptr, *dk = nullptr, *drs = nullptr;
  uint32_t *dok = nullptr, *dpath = nullptr;
  const size_t col = 32 * (size_t)n;
  hipError_t e = b.alloc((void**)&de, col);
  if (e == hipSuccess) e = b.alloc((void**)&dd, col);
  if (e == hipSuccess) e = b.alloc((void**)&dk, col);
  if (e == hipSuccess) e = b.alloc((void**)&drs, 2 * col);
  if (e == hipSuccess) e = b.alloc((void**)&dok, 4 * (size_t)n);
  if (e == hipSuccess) e = b.alloc((void**)&dpath, 4 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(de, e_be, col, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dd, d_be, col, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dk, k_be, col, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(drs, 0xA5, 2 * col);
  if (e == hipSuccess) {
    k_probe_sign_with_k<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(de, dd, dk, g_gtab, drs, dok, dpath, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_rs, drs, 2 * col, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_ok, dok, 4 * (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_path, dpath, 4 * (size_t)n, hipMemcpyDeviceToHost);
  return (int)e;
}

}  // extern "C"
