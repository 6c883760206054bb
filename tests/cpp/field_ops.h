// field_ops.h -- TEST INFRASTRUCTURE ONLY.
//
// One wrapper per operation of the CPU-tested arithmetic headers (fe29.h,
// fes.h, p256_algo.h, sec1.h): op_NAME(in, out) reads its operands from `in`
// (9 words per field element, extras as single words) and writes every result
// to `out`.  The same wrappers are compiled twice:
//   * by hipcc into tests/cpp/libfield_probe.so (field_probe.hip), one lane
//     per case, with the product library's flags -- the device build of the
//     headers: opaque_u32 / opaque_limb / fs_keep are inline asm there,
//     and_xor is a builtin, and LLVM picks the multiply-add forms;
//   * by g++ into tests/cpp/libalgo_harness.so (algo_harness.cpp), a loop
//     over the cases.
// tests/test_gpu_field_probe.py asserts that the two agree limb for limb and
// that both equal Python integers.
//
// FIELD_OPS(X): X(name, words in per case, words out per case).
#pragma once
#include <cstdint>
#include <cstring>

#include "../../simple_pbft_amd/csrc/sec1.h"  // p256_algo.h, fes.h, fe29.h

namespace field_ops {
using namespace pbftv;

PBFTV_HD void ld(fe& d, const uint32_t* s) {
  PBFTV_UNROLL for (int i = 0; i < 9; ++i) d.v[i] = s[i];
}
PBFTV_HD void st(uint32_t* d, const fe& s) {
  PBFTV_UNROLL for (int i = 0; i < 9; ++i) d[i] = s.v[i];
}
PBFTV_HD void ld4(xyzz_s& A, const uint32_t* s) {
  ld(A.x, s);
  ld(A.y, s + 9);
  ld(A.zz, s + 18);
  ld(A.zzz, s + 27);
}
PBFTV_HD void st4(uint32_t* d, const xyzz_s& A) {
  st(d, A.x);
  st(d + 9, A.y);
  st(d + 18, A.zz);
  st(d + 27, A.zzz);
}

// ---- fes.h products -----------------------------------------------------------
PBFTV_HD void op_fs_mul(const uint32_t* in, uint32_t* out) {
  fe a, b, r;
  ld(a, in);
  ld(b, in + 9);
  fs_mul(r, a, b);
  st(out, r);
  fs_mul(a, a, b);  // the output is the first operand
  st(out + 9, a);
}
PBFTV_HD void op_fs_sqr(const uint32_t* in, uint32_t* out) {
  fe a, r;
  ld(a, in);
  fs_sqr(r, a);
  st(out, r);
  fs_sqr(a, a);
  st(out + 9, a);
}
PBFTV_HD void op_fs_mul2_add(const uint32_t* in, uint32_t* out) {
  fe a, b, c, d, r;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  ld(d, in + 27);
  fs_mul2_add(r, a, b, c, d);
  st(out, r);
  fs_mul2_add(c, a, b, c, d);  // as xyzz_madd_s_flip: the output is c
  st(out + 9, c);
}
// out: r distinct | r is b | r is c
PBFTV_HD void op_fs_sqr_sub2(const uint32_t* in, uint32_t* out) {
  fe a, b, c, r;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  fs_sqr_sub2(r, a, b, c);
  st(out, r);
  fe b2 = b, c2 = c;
  fs_sqr_sub2(b2, a, b2, c);
  st(out + 9, b2);
  fs_sqr_sub2(c2, a, b, c2);
  st(out + 18, c2);
}
PBFTV_HD void op_fs_sqr_mul_add(const uint32_t* in, uint32_t* out) {
  fe a, b, c, r;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  fs_sqr_mul_add(r, a, b, c);
  st(out, r);
}
// out: r1, r2 distinct | r1 is a1, r2 is b2 | r1 is b1, r2 is a2
PBFTV_HD void op_fs_mul_x2(const uint32_t* in, uint32_t* out) {
  fe a1, b1, a2, b2, r1, r2;
  ld(a1, in);
  ld(b1, in + 9);
  ld(a2, in + 18);
  ld(b2, in + 27);
  fs_mul_x2(r1, a1, b1, r2, a2, b2);
  st(out, r1);
  st(out + 9, r2);
  fe x = a1, y = b2;
  fs_mul_x2(x, x, b1, y, a2, y);
  st(out + 18, x);
  st(out + 27, y);
  x = b1;
  y = a2;
  fs_mul_x2(x, a1, x, y, y, b2);
  st(out + 36, x);
  st(out + 45, y);
}
// in: a, b, c, e, f.  out: distinct | r1 is b, r2 is e | r1 is c, r2 is f
PBFTV_HD void op_fs_sqr_sub2_mul(const uint32_t* in, uint32_t* out) {
  fe a, b, c, e, f, r1, r2;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  ld(e, in + 27);
  ld(f, in + 36);
  fs_sqr_sub2_mul(r1, a, b, c, r2, e, f);
  st(out, r1);
  st(out + 9, r2);
  fe x = b, y = e;
  fs_sqr_sub2_mul(x, a, x, c, y, y, f);
  st(out + 18, x);
  st(out + 27, y);
  x = c;
  y = f;
  fs_sqr_sub2_mul(x, a, b, x, y, e, y);
  st(out + 36, x);
  st(out + 45, y);
}
// in: a, b, c, d, e, f.  out: distinct | r1 is c, r2 is e (xyzz_madd_s_flip_pair's call)
PBFTV_HD void op_fs_mul2_add_mul(const uint32_t* in, uint32_t* out) {
  fe a, b, c, d, e, f, r1, r2;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  ld(d, in + 27);
  ld(e, in + 36);
  ld(f, in + 45);
  fs_mul2_add_mul(r1, a, b, c, d, r2, e, f);
  st(out, r1);
  st(out + 9, r2);
  fe x = c, y = e;
  fs_mul2_add_mul(x, a, b, x, d, y, y, f);
  st(out + 18, x);
  st(out + 27, y);
}

// ---- fes.h helpers ------------------------------------------------------------
// out: fs_norm | fs_canon | fs_is_zero
PBFTV_HD void op_fs_helpers(const uint32_t* in, uint32_t* out) {
  fe a, r;
  ld(a, in);
  fs_norm(r, a);
  st(out, r);
  fs_canon(r, a);
  st(out + 9, r);
  out[18] = fs_is_zero(a) ? 1u : 0u;
}

// ---- fes.h point steps ----------------------------------------------------------
// in: acc (x, y, zz, zzz), x2, y2
PBFTV_HD void op_xyzz_madd_s_flip(const uint32_t* in, uint32_t* out) {
  xyzz_s A;
  fe x2, y2;
  ld4(A, in);
  ld(x2, in + 36);
  ld(y2, in + 45);
  xyzz_madd_s_flip(A, x2, y2);
  st4(out, A);
}
// in: x0, y0, x1, y1, flip
PBFTV_HD void op_xyzz_aff_aff_s(const uint32_t* in, uint32_t* out) {
  fe x0, y0, x1, y1;
  ld(x0, in);
  ld(y0, in + 9);
  ld(x1, in + 18);
  ld(y1, in + 27);
  xyzz_s A;
  xyzz_aff_aff_s(A, x0, y0, x1, y1, in[36] != 0);
  st4(out, A);
}
// in: acc, x2, y2, rz.  out: d | fs_is_zero(d)
PBFTV_HD void op_xyzz_last_s(const uint32_t* in, uint32_t* out) {
  xyzz_s A;
  fe x2, y2, rz, d;
  ld4(A, in);
  ld(x2, in + 36);
  ld(y2, in + 45);
  ld(rz, in + 54);
  xyzz_last_s L;
  xyzz_last_prep_s(L, A, x2, y2);
  xyzz_last_d_s(d, L, rz);
  st(out, d);
  out[9] = fs_is_zero(d) ? 1u : 0u;
}

// ---- fe29.h ---------------------------------------------------------------------
PBFTV_HD void op_fe_mul(const uint32_t* in, uint32_t* out) {
  fe a, b, r;
  ld(a, in);
  ld(b, in + 9);
  fe_mul(r, a, b);
  st(out, r);
}
PBFTV_HD void op_fe_sqr(const uint32_t* in, uint32_t* out) {
  fe a, r;
  ld(a, in);
  fe_sqr(r, a);
  st(out, r);
}
PBFTV_HD void op_fe_mul2_add(const uint32_t* in, uint32_t* out) {
  fe a, b, c, d, r;
  ld(a, in);
  ld(b, in + 9);
  ld(c, in + 18);
  ld(d, in + 27);
  fe_mul2_add(r, a, b, c, d);
  st(out, r);
}
PBFTV_HD void op_fe_sub(const uint32_t* in, uint32_t* out) {
  fe a, b, r;
  ld(a, in);
  ld(b, in + 9);
  fe_sub(r, a, b);
  st(out, r);
}
// in: a, k
PBFTV_HD void op_fe_mul_small(const uint32_t* in, uint32_t* out) {
  fe a, r;
  ld(a, in);
  fe_mul_small(r, a, in[9]);
  st(out, r);
}
PBFTV_HD void op_fe_canon(const uint32_t* in, uint32_t* out) {
  fe a, r;
  ld(a, in);
  fe_canon(r, a);
  st(out, r);
}
PBFTV_HD void op_fn_mul(const uint32_t* in, uint32_t* out) {
  fe a, b, r;
  ld(a, in);
  ld(b, in + 9);
  fn_mul(r, a, b);
  st(out, r);
}
// out: the root | the flag
PBFTV_HD void op_fe_sqrt_p(const uint32_t* in, uint32_t* out) {
  fe t, y;
  ld(t, in);
  const bool ok = fe_sqrt_p(y, t);
  st(out, y);
  out[9] = ok ? 1u : 0u;
}
// in: the entry's 16 words, neg.  out: x | y
PBFTV_HD void op_entry_to_fe_cneg(const uint32_t* in, uint32_t* out) {
  uint32_t e[16];
  PBFTV_UNROLL for (int i = 0; i < 16; ++i) e[i] = in[i];
  fe x, y;
  entry_to_fe_cneg(x, y, e, in[16] != 0);
  st(out, x);
  st(out + 9, y);
}

}  // namespace field_ops

#define FIELD_OPS(X)          \
  X(fs_mul, 18, 18)           \
  X(fs_sqr, 9, 18)            \
  X(fs_mul2_add, 36, 18)      \
  X(fs_sqr_sub2, 27, 27)      \
  X(fs_sqr_mul_add, 27, 9)    \
  X(fs_mul_x2, 36, 54)        \
  X(fs_sqr_sub2_mul, 45, 54)  \
  X(fs_mul2_add_mul, 54, 36)  \
  X(fs_helpers, 9, 19)        \
  X(xyzz_madd_s_flip, 54, 36) \
  X(xyzz_aff_aff_s, 37, 36)   \
  X(xyzz_last_s, 63, 10)      \
  X(fe_mul, 18, 9)            \
  X(fe_sqr, 9, 9)             \
  X(fe_mul2_add, 36, 9)       \
  X(fe_sub, 18, 9)            \
  X(fe_mul_small, 10, 9)      \
  X(fe_canon, 9, 9)           \
  X(fn_mul, 18, 9)            \
  X(fe_sqrt_p, 9, 10)         \
  X(entry_to_fe_cneg, 17, 18)

// the table itself, for the callers that size the buffers (hb_words, fp_words): 0, or -1 for an unknown name
static inline int field_op_words(const char* name, int* in, int* out) {
#define FIELD_WORDS(n, IN, OUT) \
  if (!std::strcmp(name, #n)) { \
    *in = IN;                   \
    *out = OUT;                 \
    return 0;                   \
  }
  FIELD_OPS(FIELD_WORDS)
#undef FIELD_WORDS
  return -1;
}
