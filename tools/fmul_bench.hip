// Field-multiplication throughput microbenchmark for gfx950: cycles per wave
// per fe_mul for the product/reduction schedules in fe29.h, with K
// independent dependency chains per lane (ILP) and LDS-limited occupancy.
// Measurement tool for DESIGN.md §3 (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I simple_pbft_amd/csrc tools/fmul_bench.hip -o tools/fmul_bench
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "fes.h"

using namespace pbftv;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1);} } while (0)

template <int V>
__device__ __forceinline__ void mul_v(fe& r, const fe& a, const fe& b) {
  if constexpr (V == 0) fe_mul(r, a, b);
  else if constexpr (V == 1) fe_mul_rows_then_reduce(r, a, b);
  else if constexpr (V == 2) fe_sqr(r, a);
  else if constexpr (V == 3) fe_sqr_il(r, a);
  // signed-limb products (fes.h): the kept row schedule against the column-order upper half
  else if constexpr (V == 4) fs_mul_rows(r, a, b);
  else if constexpr (V == 5) fs_mul(r, a, b);
  else if constexpr (V == 6) fs_sqr_rows(r, a);
  else fs_sqr(r, a);
}

// the products of three and four operands: a is the chain, c the chain's value
// of the iteration before (so that no product of two operands stays the same
// from one iteration to the next and leaves the loop), b and d are fixed
template <int V>
__device__ __forceinline__ void mul_w(fe& r, const fe& a, const fe& b, const fe& c, const fe& d) {
  if constexpr (V == 8) fs_sqr_sub2_rows(r, a, b, c);
  else if constexpr (V == 9) fs_sqr_sub2(r, a, b, c);
  else if constexpr (V == 10) fs_mul2_add_rows(r, a, b, c, d);
  else if constexpr (V == 11) fs_mul2_add(r, a, b, c, d);
  else if constexpr (V == 12) fs_sqr_mul_add_rows(r, a, b, c);
  else fs_sqr_mul_add(r, a, b, c);
}

// occupancy limited by dynamic LDS: lds_bytes per 256-thread block
template <int V, int K>
__global__ void __launch_bounds__(256) kbench(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int iters) {
  extern __shared__ uint32_t pad[];
  const int lane = blockIdx.x * 256 + threadIdx.x;
  fe a[K], b;
  for (int l = 0; l < 9; ++l) b.v[l] = in[(lane * 7 + l) & 1023] & kMask29;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < 9; ++l) a[k].v[l] = in[(lane * 3 + 11 * k + l) & 1023] & kMask29;
  if constexpr (V < 8) {
    for (int i = 0; i < iters; ++i) {
      PBFTV_UNROLL for (int k = 0; k < K; ++k) mul_v<V>(a[k], a[k], b);
    }
  } else {
    fe c[K], d;
    for (int l = 0; l < 9; ++l) d.v[l] = in[(lane * 5 + 101 + l) & 1023] & (l < 8 ? kMask29 : 0xFFFFFFu);
    b.v[8] &= 0xFFFFFFu;
    for (int k = 0; k < K; ++k)
      for (int l = 0; l < 9; ++l) c[k].v[l] = in[(lane * 13 + 7 * k + 211 + l) & 1023] & (l < 8 ? kMask29 : 0xFFFFFFu);
    for (int i = 0; i < iters; ++i) {
      PBFTV_UNROLL for (int k = 0; k < K; ++k) {
        const fe t = a[k];
        mul_w<V>(a[k], t, b, c[k], d);
        c[k] = t;
      }
    }
    for (int k = 0; k < K; ++k) a[k].v[0] ^= c[k].v[3];
  }
  uint32_t x = 0;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < 9; ++l) x ^= a[k].v[l];
  if (threadIdx.x == 0) pad[0] = x;
  __syncthreads();
  out[lane] = x ^ pad[0];
}

template <int V, int K>
static void run(const char* name, const uint32_t* in, uint32_t* out, int waves_per_simd, int iters) {
  const int blocks = 256 * 8 * 2;
  const size_t lds = 160 * 1024 / waves_per_simd - 256;
  CHECK(hipFuncSetAttribute((const void*)kbench<V, K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  hipLaunchKernelGGL((kbench<V, K>), dim3(blocks), dim3(256), lds, 0, in, out, 2);
  CHECK(hipDeviceSynchronize());
  CHECK(hipEventRecord(a));
  hipLaunchKernelGGL((kbench<V, K>), dim3(blocks), dim3(256), lds, 0, in, out, iters);
  CHECK(hipEventRecord(b));
  CHECK(hipEventSynchronize(b));
  float ms;
  CHECK(hipEventElapsedTime(&ms, a, b));
  const double waves = blocks * 4.0;
  const double cyc = ms * 1e-3 * 2.4e9 * 1024.0 / (waves * iters * K);
  printf("%-19s K=%d waves/SIMD=%d: %8.3f ms  %6.0f SIMD-cycles per wave-op\n", name, K, waves_per_simd, ms, cyc);
}

template <int V>
static void sweep(const char* name, const uint32_t* in, uint32_t* out) {
  for (int w : {1, 2, 4}) {
    run<V, 1>(name, in, out, w, 256);
    run<V, 2>(name, in, out, w, 128);
    run<V, 4>(name, in, out, w, 64);
  }
}

int main() {
  uint32_t h[1024];
  uint32_t s = 12345;
  for (int i = 0; i < 1024; ++i) { s = s * 1664525u + 1013904223u; h[i] = s; }
  uint32_t *in, *out;
  CHECK(hipMalloc(&in, sizeof(h)));
  CHECK(hipMemcpy(in, h, sizeof(h), hipMemcpyHostToDevice));
  CHECK(hipMalloc(&out, 256 * 8 * 2 * 256 * 4));
  sweep<0>("fe_mul", in, out);
  sweep<1>("fe_mul_rows_then_reduce", in, out);
  sweep<2>("fe_sqr", in, out);
  sweep<3>("fe_sqr_il", in, out);
  sweep<4>("fs_mul_rows", in, out);
  sweep<5>("fs_mul", in, out);
  sweep<6>("fs_sqr_rows", in, out);
  sweep<7>("fs_sqr", in, out);
  sweep<8>("fs_sqr_sub2_rows", in, out);
  sweep<9>("fs_sqr_sub2", in, out);
  sweep<10>("fs_mul2_add_rows", in, out);
  sweep<11>("fs_mul2_add", in, out);
  sweep<12>("fs_sqr_mul_add_rows", in, out);
  sweep<13>("fs_sqr_mul_add", in, out);
  return 0;
}
