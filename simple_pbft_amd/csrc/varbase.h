// varbase.h -- ECDSA-P256 verification under a key that has no comb table:
// R = u1*G + u2*Q with Q the signature's OWN public key (one signature per
// lane, p256_algo.h's field and group code).
//
// Semantics are those of the registered path (p256_algo.h): 0 < r, s < n, e
// not reduced, R = u1*G + u2*Q, reject R = infinity, accept iff R.x mod n == r.
// A key that fails key_check makes the signature a 0 bit.
//
// u2*Q, fixed 4-bit signed windows.  The lane builds 1Q .. 8Q (one doubling,
// six mixed additions; Jacobian, 27 limbs each = 864 B per lane) and walks u2
// from the top: 65 digits d_i in [-7, 8], u2 = sum d_i 16^i, recoded by the
// rule of signed_digit_w (vb_recode).  Per digit: four doublings, then one
// general addition of sign(d_i) * T[|d_i| - 1].  The window is FIXED on
// purpose: the 64 lanes of a wave double four times and add once in lock
// step, where a NAF or a sliding window would make the wave pay an addition
// at every bit some lane wants one.  A zero digit and the "accumulator still
// infinity" state (the common start: the top digit is only the recoding
// carry) are lane selects on the result, not branches.
//
// u1*G, after the ladder: 17 mixed additions of the width-16 G comb entries
// (CombGeom<16>), also unchecked.
//
// Exceptional cases.  Over the integers the ladder never meets one: before
// digit i the accumulator is P*Q with P = floor(u2 / 16^(i+1)) + carry >= 0,
// and 16 P = +-d_i with |d_i| <= 8 only for P = 0.  Modulo n (Q has order n,
// 0 < u2 < n) that leaves 16 P +- d_i = n, which the sizes allow at the last
// digit only and the digits allow for exactly one scalar: u2 = n - 2 (low
// nibble F, d_0 = -1, 16 P = n - 1: the last addition is -Q + -Q).  In the G
// part an adversary who picks (r, s, e) picks u1 and u2 and CAN make a partial
// sum meet the next comb point or its negative.  Every such meeting leaves
// H == 0 in the unchecked addition, so Z3 == 0, and a zero Z is kept by every
// later doubling and addition: ONE Z == 0 test per signature after the G part
// sends it to an exact rerun (varbase_mult_exact: checked additions, a
// doubling where two points are equal, infinity where they cancel) -- the
// comb's pattern in comb2_mult.
//
// Compiled by hipcc for k_varbase (p256_varbase.hip) and by g++ for the CPU
// harness (tests/cpp/varbase_harness.cpp), which runs this same limb code.
#pragma once
#include "p256_algo.h"

#if defined(__HIPCC__)
#define PBFTV_NOUNROLL _Pragma("unroll 1")
#else
#define PBFTV_NOUNROLL
#endif

namespace pbftv {

constexpr int kVbW = 4;                                  // window bits
constexpr int kVbWin = 65;                               // digits of u2 (the 65th is the recoding carry)
constexpr int kVbEnt = 8;                                // table entries: 1Q .. 8Q
constexpr int kVbPointWords = 27;                        // x, y, z: 9 limbs each
constexpr int kVbLaneWords = kVbEnt * kVbPointWords;     // 216 words = 864 B per lane
constexpr int kVbGBits = 16;                             // geometry of the G comb this path reads
constexpr int kVbGWin = CombGeom<kVbGBits>::kWin;        // 17

// Signed 4-bit recoding of u in one 256-bit addition: with K = 0x77..7 (64
// nibbles), nibble i of t = u + K is (b_i + 7 + c_i) mod 16 and carries out
// when b_i + c_i > 8 -- signed_digit_w's rule -- so d_i = nibble_i(t) - 7 for
// i < 64, and the returned carry out of bit 255 is d_64 (0 or 1).
PBFTV_HD uint32_t vb_recode(uint32_t t[8], const uint32_t u[8]) {
  uint64_t cy = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) {
    cy += (uint64_t)u[i] + 0x77777777u;
    t[i] = (uint32_t)cy;
    cy >>= 32;
  }
  return (uint32_t)cy;
}

// the next digit from the top of t (d_63 first), t shifted up by one nibble
PBFTV_HD int vb_next_digit(uint32_t t[8]) {
  const int d = (int)(t[7] >> 28) - 7;
  PBFTV_UNROLL for (int j = 7; j > 0; --j) t[j] = (t[j] << 4) | (t[j - 1] >> 28);
  t[0] <<= 4;
  return d;
}

// the next 16-bit comb digit of w (window 0 first; the 17th reads zeros), by
// signed_digit_w<16>'s rule; w shifted down by one window
PBFTV_HD int vb_next_gdigit(uint32_t w[8], int& c) {
  const int d = (int)(w[0] & 0xFFFFu) + c;
  PBFTV_UNROLL for (int j = 0; j < 7; ++j) w[j] = (w[j] >> 16) | (w[j + 1] << 16);
  w[7] >>= 16;
  c = d > (1 << 15) ? 1 : 0;
  return d - (c << 16);
}

// d = c ? a : d by masks (a ?: between two objects becomes a load through a
// selected pointer on the device, which would put both in scratch)
PBFTV_HD void vb_sel(fe& d, bool c, const fe& a) {
  const uint32_t m = 0u - (uint32_t)c;
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) d.v[l] ^= (d.v[l] ^ a.v[l]) & m;
}

PBFTV_HD void vb_sel(jac& d, bool c, const jac& a) {
  vb_sel(d.x, c, a.x);
  vb_sel(d.y, c, a.y);
  vb_sel(d.z, c, a.z);
}

// y = neg ? -y : y, N-type either way
PBFTV_HD void vb_cneg(fe& y, bool neg) {
  fe t, ny;
  fe_neg_lazy(t, y);
  fe_norm(ny, t);
  vb_sel(y, neg, ny);
}

// T[k] = (k + 1) Q for k < 8, Q = (x, y) affine Montgomery form, handed to
// st(k, point).  (k + 1) Q never meets +-Q for 2 <= k + 1 <= 7 (order n).
template <class Store>
PBFTV_HD void vb_build_table(const fe& x, const fe& y, Store st) {
  jac cur;
  cur.x = x;
  cur.y = y;
  fe_set(cur.z, kOneP);
  st(0, cur);
  jac_double(cur, cur);
  st(1, cur);
  PBFTV_NOUNROLL for (int k = 2; k < kVbEnt; ++k) {
    jac_madd<false>(cur, x, y);
    st(k, cur);
  }
}

// acc (+)= u2 * Q, unchecked.  ld(idx, point) fetches T[idx].  inf: acc holds
// no point yet (its limbs are then don't-care values, any limbs < 2^29).
template <class LoadT>
PBFTV_HD void vb_ladder(jac& acc, bool& inf, const uint32_t u2[8], LoadT ld) {
  uint32_t t[8];
  int d = (int)vb_recode(t, u2);
  PBFTV_NOUNROLL for (int i = kVbWin - 1; i >= 0; --i) {
    if (i < kVbWin - 1) {
      d = vb_next_digit(t);
      PBFTV_NOUNROLL for (int k = 0; k < kVbW; ++k) jac_double(acc, acc);
    }
    const int a = d < 0 ? -d : d;
    jac e, s;
    ld(a > 0 ? a - 1 : 0, e);
    vb_cneg(e.y, d < 0);
    jac_add<false>(s, acc, e);
    vb_sel(s, inf, e);        // the first point is the entry itself
    vb_sel(acc, d != 0, s);   // a zero digit adds nothing
    inf = inf && d == 0;
  }
}

// acc (+)= u1 * G over the width-16 comb, unchecked.  ldg(window, idx,
// words[16]) fetches a comb entry (affine, canonical Montgomery words).
template <class LoadG>
PBFTV_HD void vb_gpart(jac& acc, bool& inf, const uint32_t u1[8], LoadG ldg) {
  uint32_t w[8];
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) w[j] = u1[j];
  int c = 0;
  PBFTV_NOUNROLL for (int i = 0; i < kVbGWin; ++i) {
    const int d = vb_next_gdigit(w, c);
    const int a = d < 0 ? -d : d;
    uint32_t ew[16];
    ldg(i, a > 0 ? a - 1 : 0, ew);
    jac e, s;
    entry_to_fe(e.x, e.y, ew);
    vb_cneg(e.y, d < 0);
    fe_set(e.z, kOneP);
    s = acc;
    jac_madd<false>(s, e.x, e.y);
    vb_sel(s, inf, e);
    vb_sel(acc, d != 0, s);
    inf = inf && d == 0;
  }
}

// The exact form: u1*G + u2*Q with every meeting handled.  false: infinity.
template <class LoadT, class LoadG>
PBFTV_HD bool varbase_mult_exact(jac& acc, const uint32_t u1[8], const uint32_t u2[8], LoadT ld, LoadG ldg) {
  bool inf = true;
  uint32_t t[8];
  int d = (int)vb_recode(t, u2);
  PBFTV_NOUNROLL for (int i = kVbWin - 1; i >= 0; --i) {
    if (i < kVbWin - 1) {
      d = vb_next_digit(t);
      if (!inf) {  // (a finite point of odd order never doubles to infinity)
        PBFTV_NOUNROLL for (int k = 0; k < kVbW; ++k) jac_double(acc, acc);
      }
    }
    if (d == 0) continue;
    jac e, s;
    ld((d < 0 ? -d : d) - 1, e);
    vb_cneg(e.y, d < 0);
    if (inf) {
      acc = e;
      inf = false;
      continue;
    }
    const int st = jac_add<true>(s, acc, e);
    if (st == 0) acc = s;
    else if (st == 1) jac_double(acc, acc);
    else inf = true;
  }
  uint32_t w[8];
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) w[j] = u1[j];
  int c = 0;
  PBFTV_NOUNROLL for (int i = 0; i < kVbGWin; ++i) {
    const int g = vb_next_gdigit(w, c);
    if (g == 0) continue;
    uint32_t ew[16];
    ldg(i, (g < 0 ? -g : g) - 1, ew);
    comb_add_entry<true>(acc, inf, g, ew);
  }
  return !inf;
}

// The fast form as the kernel runs it: ladder, G part, then the one Z test.
// Returns 1 / 0 = R finite / infinity, -1 = some step met (run the exact form).
template <class LoadT, class LoadG>
PBFTV_HD int varbase_mult_fast(jac& acc, const uint32_t u1[8], const uint32_t u2[8], LoadT ld, LoadG ldg) {
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) acc.x.v[l] = acc.y.v[l] = acc.z.v[l] = 0;
  bool inf = true;
  vb_ladder(acc, inf, u2, ld);
  vb_gpart(acc, inf, u1, ldg);
  if (inf) return 0;
  return fe_is_zero(acc.z) ? -1 : 1;
}

// One signature from its stage-1 scalars, in k_varbase's schedule.  (x, y):
// the key, affine Montgomery form (key_check's output); tab: kVbEnt points of
// scratch.  out_path (optional): bit 0 = the exact rerun ran.
template <class LoadG>
PBFTV_HD bool varbase_verify(const uint32_t u1[8], const uint32_t u2[8], const uint32_t r_w[8], const fe& x,
                             const fe& y, jac* tab, LoadG ldg, int* out_path = nullptr) {
  vb_build_table(x, y, [&](int k, const jac& p) { tab[k] = p; });
  auto ld = [&](int idx, jac& p) { p = tab[idx]; };
  jac R;
  int fin = varbase_mult_fast(R, u1, u2, ld, ldg);
  if (out_path) *out_path = fin < 0 ? 1 : 0;
  if (fin < 0) fin = varbase_mult_exact(R, u1, u2, ld, ldg) ? 1 : 0;
  return ecdsa_check(R, fin == 1, r_w);
}

// ... and from the wire values (LE words): key check, stage 1, then the above.
template <class LoadG>
PBFTV_HD bool varbase_verify_sig(const uint32_t e_w[8], const uint32_t r_w[8], const uint32_t s_w[8],
                                 const uint32_t x_w[8], const uint32_t y_w[8], jac* tab, LoadG ldg,
                                 int* out_path = nullptr) {
  if (out_path) *out_path = 0;
  fe xm, ym;
  if (!key_check(x_w, y_w, xm, ym)) return false;
  uint32_t u1[8], u2[8];
  if (!ecdsa_scalars(e_w, r_w, s_w, u1, u2)) return false;
  return varbase_verify(u1, u2, r_w, xm, ym, tab, ldg, out_path);
}

}  // namespace pbftv
