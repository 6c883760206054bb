// fs_columns_harness.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The five signed-limb products of simple_pbft_amd/csrc/fes.h in both
// schedules -- the column-order upper half the kernels run (fs_mul, ...) and
// the kept row schedule (fs_mul_rows, ...) -- compiled with g++ for
// tests/test_fs_columns.py, which checks them limb for limb against each
// other and against Python integers.  Built as a shared object for the test,
// and with -DFS_COLUMNS_MAIN as a stand-alone program (own main, for a
// -fsanitize=address,undefined build) that runs the same comparison on fixed
// edge inputs and a random stream.  Never linked into the product library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../simple_pbft_amd/csrc/fes.h"

using namespace pbftv;

namespace {

enum { OP_MUL = 0, OP_SQR = 1, OP_SQR_SUB2 = 2, OP_MUL2_ADD = 3, OP_SQR_MUL_ADD = 4, OP_COUNT = 5 };

// in: four operands of 9 limbs (a, b, c, d; an op reads the ones it takes)
void run_op(int op, bool rows, const uint32_t* in, uint32_t* out) {
  fe a, b, c, d, r;
  memcpy(a.v, in, 36);
  memcpy(b.v, in + 9, 36);
  memcpy(c.v, in + 18, 36);
  memcpy(d.v, in + 27, 36);
  memset(r.v, 0, 36);
  switch (op) {
    case OP_MUL: rows ? fs_mul_rows(r, a, b) : fs_mul(r, a, b); break;
    case OP_SQR: rows ? fs_sqr_rows(r, a) : fs_sqr(r, a); break;
    case OP_SQR_SUB2: rows ? fs_sqr_sub2_rows(r, a, b, c) : fs_sqr_sub2(r, a, b, c); break;
    case OP_MUL2_ADD: rows ? fs_mul2_add_rows(r, a, b, c, d) : fs_mul2_add(r, a, b, c, d); break;
    case OP_SQR_MUL_ADD: rows ? fs_sqr_mul_add_rows(r, a, b, c) : fs_sqr_mul_add(r, a, b, c); break;
  }
  memcpy(out, r.v, 36);
}

}  // namespace

extern "C" {

// n operand sets of 36 words each -> n results of 9 words per schedule;
// returns the number of sets whose two results differ in any limb
uint64_t h_fsc_batch(int op, uint64_t n, const uint32_t* in, uint32_t* out_cols, uint32_t* out_rows) {
  uint64_t bad = 0;
  for (uint64_t i = 0; i < n; ++i) {
    run_op(op, false, in + 36 * i, out_cols + 9 * i);
    run_op(op, true, in + 36 * i, out_rows + 9 * i);
    bad += memcmp(out_cols + 9 * i, out_rows + 9 * i, 36) != 0;
  }
  return bad;
}

// the product with the result written over its first operand (the comb's
// fs_mul(acc.zz, acc.zz, pp)): the outputs may not be stored before the last
// column has read the operands
void h_fsc_mul_inplace(const uint32_t* a, const uint32_t* b, uint32_t* r) {
  fe x, y;
  memcpy(x.v, a, 36);
  memcpy(y.v, b, 36);
  fs_mul(x, x, y);
  memcpy(r, x.v, 36);
}

// fs_sqr_sub2 (lone, rows, and paired with e f) with a result written over b
// (over = 1) or c (over = 2): limb 8 of b and c goes into the top limb after
// the reduction.  in: a, b, c, e, f; out: r1 of the three forms, then r2 = e f.
void h_fsc_sqr_sub2_over(int over, const uint32_t* in, uint32_t* out) {
  fe v[5], w[5];
  for (int k = 0; k < 5; ++k) memcpy(v[k].v, in + 9 * k, 36);
  memcpy(w, v, sizeof w);
  fs_sqr_sub2(w[over], w[0], w[1], w[2]);
  memcpy(out, w[over].v, 36);
  memcpy(w, v, sizeof w);
  fs_sqr_sub2_rows(w[over], w[0], w[1], w[2]);
  memcpy(out + 9, w[over].v, 36);
  memcpy(w, v, sizeof w);
  fe r1;
  fs_sqr_sub2_mul(r1, w[0], w[1], w[2], w[over], w[3], w[4]);  // r2 over b or c
  memcpy(out + 18, r1.v, 36);
  memcpy(out + 27, w[over].v, 36);
}

// the comb's addition (acc: X, W, ZZ, ZZZ; pt: x2, y2) on the row-schedule
// products (variant 0), on lone column chains (1) and on paired ones (2, the
// form xyzz_madd_s_flip runs)
void h_fsc_madd(int variant, uint32_t* acc, const uint32_t* pt) {
  xyzz_s a;
  fe x2, y2;
  memcpy(a.x.v, acc, 36); memcpy(a.y.v, acc + 9, 36); memcpy(a.zz.v, acc + 18, 36); memcpy(a.zzz.v, acc + 27, 36);
  memcpy(x2.v, pt, 36);
  memcpy(y2.v, pt + 9, 36);
  if (variant == 1) {
    xyzz_madd_s_flip_lone(a, x2, y2);
  } else if (variant == 2) {
    xyzz_madd_s_flip(a, x2, y2);
  } else {
    fe u2, s2, p, r, pp, ppp, q, t, x3;
    fs_mul_rows(u2, x2, a.zz);
    fs_mul_rows(s2, y2, a.zzz);
    fs_sub(p, u2, a.x);
    fs_sub(r, s2, a.y);
    fs_sqr_rows(pp, p);
    fs_mul_rows(ppp, p, pp);
    fs_mul_rows(q, a.x, pp);
    fs_sqr_sub2_rows(x3, r, ppp, q);
    fs_sub(t, x3, q);
    fs_mul2_add_rows(a.y, r, t, a.y, ppp);
    fs_mul_rows(a.zz, a.zz, pp);
    fs_mul_rows(a.zzz, a.zzz, ppp);
    a.x = x3;
  }
  memcpy(acc, a.x.v, 36); memcpy(acc + 9, a.y.v, 36); memcpy(acc + 18, a.zz.v, 36); memcpy(acc + 27, a.zzz.v, 36);
}

}  // extern "C"

#if defined(FS_COLUMNS_MAIN)
namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd32() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// S-type: limbs 0..7 in [0, 2^29), limb 8 signed below 2^25.5 in magnitude
void rnd_s(uint32_t* l) {
  for (int i = 0; i < 8; ++i) l[i] = rnd32() & kMask29;
  l[8] = (uint32_t)((int32_t)rnd32() >> 7);
}
// D-type: a difference of two S-type values
void rnd_d(uint32_t* l) {
  uint32_t x[9], y[9];
  rnd_s(x);
  rnd_s(y);
  for (int i = 0; i < 9; ++i) l[i] = x[i] - y[i];
}

int check(int op, const uint32_t* in, const char* what) {
  uint32_t a[9], b[9];
  run_op(op, false, in, a);
  run_op(op, true, in, b);
  if (memcmp(a, b, 36) != 0) {
    fprintf(stderr, "mismatch: op %d, %s\n", op, what);
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 200000;
  int bad = 0;
  uint32_t in[36];
  const uint32_t top = kMask29, neg = 0u - kMask29;
  // every limb at +-(2^29 - 1), in every sign pairing of the operands, and zero
  for (int op = 0; op < OP_COUNT; ++op) {
    for (int signs = 0; signs < 16; ++signs) {
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 9; ++i) in[9 * k + i] = (signs >> k) & 1 ? neg : top;
      bad += check(op, in, "all limbs at the bound");
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 9; ++i) in[9 * k + i] = ((signs >> k) ^ i) & 1 ? neg : top;
      bad += check(op, in, "alternating limbs at the bound");
    }
    memset(in, 0, sizeof in);
    bad += check(op, in, "zero");
    // limb 8 at its signed extremes on random lower limbs
    for (int it = 0; it < 64; ++it) {
      for (int k = 0; k < 4; ++k) {
        rnd_s(in + 9 * k);
        in[9 * k + 8] = (it >> k) & 1 ? 0u - ((1u << 26) - 1) : (1u << 26) - 1;
      }
      bad += check(op, in, "limb 8 at its extremes");
    }
    for (int it = 0; it < n_random; ++it) {
      for (int k = 0; k < 4; ++k) ((it >> k) & 1 ? rnd_d : rnd_s)(in + 9 * k);
      if (op == OP_SQR_MUL_ADD) {  // b, c S-type
        rnd_s(in + 9);
        rnd_s(in + 18);
      }
      bad += check(op, in, "random");
    }
  }
  printf("fs_columns: %d mismatches\n", bad);
  return bad != 0;
}
#endif
