// field_probe.hip -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_field_probe.py).
//
// The latency path's field arithmetic, one operation per entry point, as the
// device runs it: rows.h (one field element per 16-lane row), the quad schedule
// and fmont_lane of verify_kernels.h, and the CPU-tested headers as hipcc
// compiles them (field_ops.h).  Built to tests/cpp/libfield_probe.so with the
// product library's flags, so the compiler's choices are the product's; it does
// not link libpbftv.so and the product never loads it.
//
// Every entry point takes host arrays and a case count, allocates, copies,
// launches, synchronises and frees on its own, and returns the hipError_t
// (-1: an argument out of range).  Shapes:
//   rows:  one wave per case, 64 words per value (all 64 lanes, so lanes 9..15
//          of every row are visible); the four rows carry four different
//          cases where the operation is per-row;
//   quads: one quad per case, role = threadIdx.x & 3, 16 cases per wave;
//   lanes: one lane per case.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../simple_pbft_amd/csrc/verify_kernels.h"
#include "field_ops.h"

using namespace pbftv;

namespace {

// in: n cases of IN words, out: n cases of OUT words; `per` cases per 64-lane block
template <class K>
int launch(K kern, const uint32_t* in, size_t IN, uint32_t* out, size_t OUT, int n, int per) {
  if (n <= 0 || !in || !out) return -1;
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, (size_t)n * IN * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * OUT * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * IN * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, (size_t)n * OUT * 4);
  if (e == hipSuccess) {
    kern<<<dim3((unsigned)((n + per - 1) / per)), dim3(64)>>>(din, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * OUT * 4, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

// ---- A. rows: value k of wave w is in[(w K + k) 64 + lane] -------------------
#define ROW_IO(K, M)                                                  \
  const int lane = (int)threadIdx.x;                                  \
  const uint32_t* src = in + (size_t)blockIdx.x * (K) * 64 + lane;    \
  uint32_t* dst = out + (size_t)blockIdx.x * (M) * 64 + lane;         \
  if ((int)blockIdx.x >= n) return;                                   \
  const RowCtx c = row_ctx()

__global__ __launch_bounds__(64) void k_row_mul(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(2, 1);
  dst[0] = row_mul(c, src[0], src[64]);
}

__global__ __launch_bounds__(64) void k_row_norm(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(1, 1);
  dst[0] = row_norm(c, src[0]);
}

// in: x, v0..v3.  out: g[0..3] of gather4(x), sel4(v0..v3)
__global__ __launch_bounds__(64) void k_gather_sel(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(5, 5);
  uint32_t g[4];
  gather4(g, src[0]);
  for (int k = 0; k < 4; ++k) dst[k * 64] = g[k];
  dst[4 * 64] = sel4(c, src[64], src[128], src[192], src[256]);
}

// in: A (x, y, zz, zzz), B, rm.  out: the sum, rz
__global__ __launch_bounds__(64) void k_xyzz_add_rows(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(9, 5);
  const xyzz_r A{src[0], src[64], src[128], src[192]}, B{src[256], src[320], src[384], src[448]};
  xyzz_r r;
  uint32_t rz;
  xyzz_add_rows(c, r, rz, A, B, src[512]);
  dst[0] = r.x;
  dst[64] = r.y;
  dst[128] = r.zz;
  dst[192] = r.zzz;
  dst[256] = rz;
}

// in: gx, gy, qx, qy (pair layout).  out: S
__global__ __launch_bounds__(64) void k_mmadd_pairs(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(4, 4);
  xyzz_r S;
  mmadd_pairs(c, S, src[0], src[64], src[128], src[192]);
  dst[0] = S.x;
  dst[64] = S.y;
  dst[128] = S.zz;
  dst[192] = S.zzz;
}

// in: A, B, rz.  out: the verdict, exc (every lane)
__global__ __launch_bounds__(64) void k_xyzz_add_check_rows(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(9, 2);
  const xyzz_r A{src[0], src[64], src[128], src[192]}, B{src[256], src[320], src[384], src[448]};
  bool exc;
  const bool ok = xyzz_add_check_rows(c, exc, A, B, src[512]);
  dst[0] = ok ? 1u : 0u;
  dst[64] = exc ? 1u : 0u;
}

// in: x.  out: row_is_zero (every lane), row_to_fe's nine limbs (every lane)
__global__ __launch_bounds__(64) void k_row_zero_fe(const uint32_t* in, uint32_t* out, int n) {
  ROW_IO(1, 10);
  (void)c;
  const uint32_t x = src[0];
  dst[0] = row_is_zero(x) ? 1u : 0u;
  fe d;
  row_to_fe(d, x);
  for (int l = 0; l < 9; ++l) dst[(1 + l) * 64] = d.v[l];
}

// window 0 of a table of `ents` entries; digs: one signed digit per row (4 per wave).  out: x, y
constexpr int kProbeW = 11;
__global__ __launch_bounds__(64) void k_row_entry(const uint4* tab, int ents, const int32_t* digs, uint32_t* out,
                                                  int n) {
  if ((int)blockIdx.x >= n) return;
  const int lane = (int)threadIdx.x;
  int d = digs[blockIdx.x * 4 + (lane >> 4)];
  const int ad = d < 0 ? -d : d;
  if (ad > ents) d = 0;  // (the host entry refuses such a digit: never read past the table)
  uint32_t x, y;
  row_entry<kProbeW>(tab, 0, d, lane & 15, x, y);
  out[(size_t)blockIdx.x * 128 + lane] = x;
  out[(size_t)blockIdx.x * 128 + 64 + lane] = y;
}

// ---- B. quads: case q of a block is lanes 4q..4q+3 ---------------------------
// (a lane past the last case recomputes the last case and stores nothing: the
// DPP moves need every lane of a quad)
#define QUAD_IO(IN, OUT)                                                   \
  const int role = (int)(threadIdx.x & 3u);                                \
  const int cs = (int)(blockIdx.x * 16 + (threadIdx.x >> 2));              \
  const bool live = cs < n;                                                \
  const uint32_t* src = in + (size_t)(live ? cs : n - 1) * (IN);           \
  uint32_t* dst = out + ((size_t)(live ? cs : n - 1) * 4 + role) * (OUT)

// in: a0, b0, .., a3, b3.  out per lane: the product
__global__ __launch_bounds__(64) void k_quad_mul(const uint32_t* in, uint32_t* out, int n) {
  QUAD_IO(72, 9);
  fe v[8], p;
  for (int k = 0; k < 8; ++k) field_ops::ld(v[k], src + 9 * k);
  quad_mul(p, role, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
  if (live) field_ops::st(dst, p);
}

// in: gx, gy, qx, qy, rm.  out per lane: x, y, zz, zzz, rz
__global__ __launch_bounds__(64) void k_quad_mmadd(const uint32_t* in, uint32_t* out, int n) {
  QUAD_IO(45, 45);
  fe v[5], rz;
  for (int k = 0; k < 5; ++k) field_ops::ld(v[k], src + 9 * k);
  xyzz_s r;
  quad_mmadd_xyzz(r, rz, role, v[0], v[1], v[2], v[3], v[4]);
  if (live) {
    field_ops::st4(dst, r);
    field_ops::st(dst + 36, rz);
  }
}

// in: P, Q, rm, qinf.  out per lane: x, y, zz, zzz, rz
__global__ __launch_bounds__(64) void k_quad_add(const uint32_t* in, uint32_t* out, int n) {
  QUAD_IO(82, 45);
  xyzz_s P, Q, r;
  fe rm, rz;
  field_ops::ld4(P, src);
  field_ops::ld4(Q, src + 36);
  field_ops::ld(rm, src + 72);
  quad_xyzz_add(r, rz, role, P, Q, rm, src[81] != 0);
  if (live) {
    field_ops::st4(dst, r);
    field_ops::st(dst + 36, rz);
  }
}

// in: P, Q, rz.  out per lane: the verdict, exc
__global__ __launch_bounds__(64) void k_quad_add_check(const uint32_t* in, uint32_t* out, int n) {
  QUAD_IO(81, 2);
  xyzz_s P, Q;
  fe rz;
  field_ops::ld4(P, src);
  field_ops::ld4(Q, src + 36);
  field_ops::ld(rz, src + 72);
  bool exc;
  const bool ok = quad_xyzz_add_check(exc, role, P, Q, rz);
  if (live) {
    dst[0] = ok ? 1u : 0u;
    dst[1] = exc ? 1u : 0u;
  }
}

// in: a, b.  The modulus by lane as wave_scalars picks it: lanes 0, 1 of a quad
// mod n with kNPrime, lanes 2, 3 mod p with 1.
__global__ __launch_bounds__(64) void k_fmont_lane(const uint32_t* in, uint32_t* out, int n) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= n) return;
  const bool modn = (threadIdx.x & 3u) < 2u;
  fe a, b, m, nmod, pmod, r;
  field_ops::ld(a, in + (size_t)i * 18);
  field_ops::ld(b, in + (size_t)i * 18 + 9);
  fe_set(nmod, kN);
  fe_set(pmod, kP);
  for (int l = 0; l < 9; ++l) m.v[l] = modn ? nmod.v[l] : pmod.v[l];
  fmont_lane(r, a, b, m, modn ? kNPrime : 1u);
  field_ops::st(out + (size_t)i * 9, r);
}

// wave_scalars / wave_scalars_lds themselves (one wave per case; 0 < r, s < n as their callers
// check): the one product step that runs fmont_lane mod n and mod p side by side, with the
// per-lane choice of modulus and digit constant as the kernels make it.
// in: e, r, s (8 LE words each).  out: u1, u2 (8 words each), rm, rnm (9 limbs each), rn_ok;
// then wave_scalars_lds's u1, u2, rm
__global__ __launch_bounds__(64) void k_wave_scalars(const uint32_t* in, uint32_t* out, int n) {
  __shared__ uint32_t su1[8], su2[8], srm[9];
  if ((int)blockIdx.x >= n) return;
  const uint32_t* src = in + (size_t)blockIdx.x * 24;
  uint32_t* dst = out + (size_t)blockIdx.x * 60;
  uint32_t e[8], r[8], s[8], u1[8], u2[8];
  for (int k = 0; k < 8; ++k) {
    e[k] = src[k];
    r[k] = src[8 + k];
    s[k] = src[16 + k];
  }
  fe rm, rnm;
  bool rn_ok;
  wave_scalars(e, r, s, u1, u2, rm, rnm, rn_ok);
  wave_scalars_lds(e, r, s, su1, su2, srm);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < 8; ++k) {
      dst[k] = u1[k];
      dst[8 + k] = u2[k];
      dst[35 + k] = su1[k];
      dst[43 + k] = su2[k];
    }
    field_ops::st(dst + 16, rm);
    field_ops::st(dst + 25, rnm);
    dst[34] = rn_ok ? 1u : 0u;
    for (int l = 0; l < 9; ++l) dst[51 + l] = srm[l];
  }
}

// ---- C. the CPU-tested headers, one lane per case ----------------------------
#define FIELD_KERNEL(name, IN, OUT)                                                             \
  __global__ __launch_bounds__(64) void k_op_##name(const uint32_t* in, uint32_t* out, int n) { \
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);                                         \
    if (i < n) field_ops::op_##name(in + (size_t)i * (IN), out + (size_t)i * (OUT));            \
  }
FIELD_OPS(FIELD_KERNEL)

}  // namespace

extern "C" {

int fp_row_mul(const uint32_t* in, uint32_t* out, int n) { return launch(k_row_mul, in, 128, out, 64, n, 1); }
int fp_row_norm(const uint32_t* in, uint32_t* out, int n) { return launch(k_row_norm, in, 64, out, 64, n, 1); }
int fp_gather_sel(const uint32_t* in, uint32_t* out, int n) { return launch(k_gather_sel, in, 320, out, 320, n, 1); }
int fp_xyzz_add_rows(const uint32_t* in, uint32_t* out, int n) {
  return launch(k_xyzz_add_rows, in, 576, out, 320, n, 1);
}
int fp_mmadd_pairs(const uint32_t* in, uint32_t* out, int n) { return launch(k_mmadd_pairs, in, 256, out, 256, n, 1); }
int fp_xyzz_add_check_rows(const uint32_t* in, uint32_t* out, int n) {
  return launch(k_xyzz_add_check_rows, in, 576, out, 128, n, 1);
}
int fp_row_zero_fe(const uint32_t* in, uint32_t* out, int n) { return launch(k_row_zero_fe, in, 64, out, 640, n, 1); }

// table: `ents` entries of 16 words; digs: 4 n signed digits, |d| <= ents; out: n x (x, y) x 64 lanes
int fp_row_entry(const uint32_t* table, int ents, const int32_t* digs, uint32_t* out, int n) {
  if (n <= 0 || ents <= 0 || ents > CombGeom<kProbeW>::ent(0) || !table || !digs || !out) return -1;
  for (int i = 0; i < 4 * n; ++i)
    if (digs[i] > ents || digs[i] < -ents) return -1;
  uint4* dtab = nullptr;
  int32_t* dd = nullptr;
  uint32_t* dout = nullptr;
  hipError_t e = hipMalloc(&dtab, (size_t)ents * 64);
  if (e == hipSuccess) e = hipMalloc(&dd, (size_t)n * 16);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 512);
  if (e == hipSuccess) e = hipMemcpy(dtab, table, (size_t)ents * 64, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dd, digs, (size_t)n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_row_entry<<<dim3((unsigned)n), dim3(64)>>>(dtab, ents, dd, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 512, hipMemcpyDeviceToHost);
  if (dtab) (void)hipFree(dtab);
  if (dd) (void)hipFree(dd);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

int fp_quad_mul(const uint32_t* in, uint32_t* out, int n) { return launch(k_quad_mul, in, 72, out, 36, n, 16); }
int fp_quad_mmadd(const uint32_t* in, uint32_t* out, int n) { return launch(k_quad_mmadd, in, 45, out, 180, n, 16); }
int fp_quad_add(const uint32_t* in, uint32_t* out, int n) { return launch(k_quad_add, in, 82, out, 180, n, 16); }
int fp_quad_add_check(const uint32_t* in, uint32_t* out, int n) {
  return launch(k_quad_add_check, in, 81, out, 8, n, 16);
}
int fp_fmont_lane(const uint32_t* in, uint32_t* out, int n) { return launch(k_fmont_lane, in, 18, out, 9, n, 64); }

int fp_wave_scalars(const uint32_t* in, uint32_t* out, int n) { return launch(k_wave_scalars, in, 24, out, 60, n, 1); }

#define FIELD_ENTRY(name, IN, OUT) \
  int fp_##name(const uint32_t* in, uint32_t* out, int n) { return launch(k_op_##name, in, IN, out, OUT, n, 64); }
FIELD_OPS(FIELD_ENTRY)
int fp_words(const char* name, int* in, int* out) { return field_op_words(name, in, out); }

}  // extern "C"
