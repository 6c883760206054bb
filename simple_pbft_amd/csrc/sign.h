// sign.h -- deterministic ECDSA-P256 signing, one signature per lane
// (p256_algo.h's field and group code, varbase.h's G comb walk).
//
// Semantics are Go's crypto/ecdsa.Sign with the nonce of RFC 6979 §3.2
// (HMAC-SHA256 DRBG, qlen = hlen = 256, no additional data): k from (d, h1),
// R = k*G, r = R.x mod n, s = k^-1 (e + r d) mod n with e = int(h1) reduced
// mod n.  No low-S normalisation: Go does none and every verify here accepts a
// high S.  A signature the algorithm cannot produce -- d = 0 or d >= n, or no
// usable nonce among the first kSignMaxCandidates candidates, which no input
// is known to reach -- is 64 zero bytes with a 0 ok bit.
//
// The DRBG as a pass list.  Every step of §3.2 is an HMAC under the running
// key K, i.e. SHA-256 compressions from one of two midstates (ki, ko: the
// ipad and opad blocks of K already absorbed).  One UPDATE -- K = HMAC_K(V ||
// sep [|| x || h]); V = HMAC_K(V) -- is seven compressions, run by ONE loop
// around ONE instance of sha256_compress (drbg_passes), so the device code
// holds three copies of the 64 unrolled rounds, not twenty:
//   pass 0  inner, block 1: V || sep || x[0..30]     (no data: V || sep || pad)
//   pass 1  inner, block 2: x[31] || h || pad         (skipped without data)
//   pass 2  outer: ko, inner digest || pad            -> the new K
//   pass 3  K ^ ipad from the IV                      -> ki
//   pass 4  K ^ opad from the IV                      -> ko
//   pass 5  inner: ki, V || pad
//   pass 6  outer: ko, inner digest || pad            -> the new V
// A candidate (step h) is passes 5 and 6 alone.  init is two UPDATEs with
// data (sep 00, 01); the key before the first is all zeros, whose midstates
// are the constants kHmacZeroKi / kHmacZeroKo.  16 compressions to the first
// candidate.
//
// Secret data.  d, k, k^-1 and the DRBG state (K, V, the midstates) never
// steer a branch and never index memory, with the two exceptions stated here:
//   * the comb entry ADDRESS in the k*G walk is k's digit (a window has 32768
//     entries: it cannot be scanned per signature).  DESIGN.md §3.16: the GPU
//     and whoever shares it are trusted;
//   * whether a candidate was REJECTED (k = 0 or k >= n: probability 2^-32,
//     and the value is discarded) and whether the signature came out with
//     r = 0, s = 0 or Z = 0 (never, see below) decide if another round runs.
// Everything else is masks and vb_sel, as in varbase.h's ladder: the digit
// walk selects on d != 0 and on its sign, the DRBG is straight-line
// compressions, k^-1 is inv_mod_n_words_ct (fixed 25 x 30 divsteps), the
// reductions mod n are subtract-and-select.  The field inversion of Z is
// Fermat with p - 2's public bits.
//
// Compiled by hipcc for p256_sign.hip and the device probe
// (tests/cpp/sign_probe.hip) and by g++ for the CPU harness
// (tests/cpp/sign_harness.cpp), which runs this same limb code.
#pragma once
#include "sha256_block.h"
#include "varbase.h"

namespace pbftv {

constexpr int kSignMaxCandidates = 4;

// SHA-256 midstates of HMAC's ipad (36..) and opad (5c..) blocks under the
// all-zero key (a wrong word fails every DRBG comparison of tests/test_sign_cpu.py)
static constexpr uint32_t kHmacZeroKi[8] = {0xf454deadu, 0x9725214fu, 0x90daf2a0u, 0xdf1228eau,
                                            0x64e5750fu, 0xa3924181u, 0x824a932bu, 0xf8e04e32u};
static constexpr uint32_t kHmacZeroKo[8] = {0xd385480fu, 0x7abb6477u, 0x37c9c538u, 0x5dd82467u,
                                            0x8e043a72u, 0x753434b0u, 0xdeb82818u, 0x361d45a6u};

// ki, ko, v: big-endian words as SHA-256 keeps them (word 0 = bytes 0..3)
struct rfc6979_state {
  uint32_t ki[8], ko[8], v[8];
  uint32_t fresh;  // 1: no candidate taken yet (the next one needs no UPDATE)
};

// w = (digest in st) || 80 || zeros || length of (one key block + 32 bytes)
PBFTV_HD void hmac_outer_block(uint32_t w[16], const uint32_t st[8]) {
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) w[j] = st[j];
  w[8] = 0x80000000u;
  PBFTV_UNROLL for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = (64 + 32) * 8;
}

// Passes first..6 of the list above.  x, h: big-endian words (word 0 the most
// significant), read when data.  first is 0 (an UPDATE) or 5 (a candidate).
PBFTV_HD void drbg_passes(rfc6979_state& S, int first, uint32_t sep, bool data, const uint32_t x[8],
                          const uint32_t h[8]) {
  uint32_t st[8], w[16], key[8];
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) {
    st[j] = S.ki[j];
    w[j] = S.v[j];
    key[j] = 0;
  }
  if (first == 0 && data) {
    w[8] = (sep << 24) | (x[0] >> 8);
    PBFTV_UNROLL for (int j = 1; j < 8; ++j) w[8 + j] = (x[j - 1] << 24) | (x[j] >> 8);
  } else {
    w[8] = first == 0 ? (sep << 24) | 0x00800000u : 0x80000000u;
    PBFTV_UNROLL for (int j = 9; j < 15; ++j) w[j] = 0;
    w[15] = first == 0 ? (64 + 33) * 8 : (64 + 32) * 8;
  }
  PBFTV_NOUNROLL for (int pass = first; pass < 7; ++pass) {
    if (pass == 1 && !data) continue;
    sha256_compress(st, w);
    if (pass == 0 && data) {
      w[0] = (x[7] << 24) | (h[0] >> 8);
      PBFTV_UNROLL for (int j = 1; j < 8; ++j) w[j] = (h[j - 1] << 24) | (h[j] >> 8);
      w[8] = (h[7] << 24) | 0x00800000u;
      PBFTV_UNROLL for (int j = 9; j < 15; ++j) w[j] = 0;
      w[15] = (64 + 97) * 8;
    } else if (pass <= 1 || pass == 5) {  // an inner digest: on to its outer hash
      hmac_outer_block(w, st);
      PBFTV_UNROLL for (int j = 0; j < 8; ++j) st[j] = S.ko[j];
    } else if (pass == 2 || pass == 3) {  // 2: st is the new K; 3: st is its ki
      const uint32_t pad = pass == 2 ? 0x36363636u : 0x5c5c5c5cu;
      PBFTV_UNROLL for (int j = 0; j < 8; ++j) {
        if (pass == 2) key[j] = st[j];
        else S.ki[j] = st[j];
        w[j] = key[j] ^ pad;
        w[8 + j] = pad;
        st[j] = kSha256Iv[j];
      }
    } else if (pass == 4) {  // st is the new ko; V's inner hash under the new key
      PBFTV_UNROLL for (int j = 0; j < 8; ++j) {
        S.ko[j] = st[j];
        st[j] = S.ki[j];
        w[j] = S.v[j];
      }
      w[8] = 0x80000000u;
      PBFTV_UNROLL for (int j = 9; j < 15; ++j) w[j] = 0;
      w[15] = (64 + 32) * 8;
    } else {  // pass 6
      PBFTV_UNROLL for (int j = 0; j < 8; ++j) S.v[j] = st[j];
    }
  }
}

// a >= b over LE words, as a mask-free borrow chain (no early exit)
PBFTV_HD bool words_ge_ct(const uint32_t a[8], const uint32_t b[8]) {
  uint64_t br = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) br = ((uint64_t)a[i] - b[i] - br) >> 63;
  return br == 0;
}

// r = a >= n ? a - n : a (LE words, a < 2n), by a mask
PBFTV_HD void words_cond_sub_n(uint32_t r[8], const uint32_t a[8]) {
  uint32_t t[8];
  uint64_t br = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)a[i] - kN32[i] - br;
    t[i] = (uint32_t)x;
    br = x >> 63;
  }
  const uint32_t keep = 0u - (uint32_t)br;  // borrow: a < n
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) r[i] = t[i] ^ ((t[i] ^ a[i]) & keep);
}

// 0 < d < n
PBFTV_HD bool sign_scalar_ok(const uint32_t d[8]) {
  uint32_t o = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) o |= d[i];
  return (o != 0) & !words_ge_ct(d, kN32);
}

// RFC 6979 §3.2 steps b..g.  d_words: the private key x, h1_words: the 32-byte
// hash as an integer; both LE words.  bits2octets(h1) is h1 - n when h1 >= n
// (2^256 < 2n).
PBFTV_HD void rfc6979_init(rfc6979_state& S, const uint32_t d_words[8], const uint32_t h1_words[8]) {
  uint32_t hr[8], x[8], h[8];
  words_cond_sub_n(hr, h1_words);
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) {
    x[j] = d_words[7 - j];
    h[j] = hr[7 - j];
    S.ki[j] = kHmacZeroKi[j];
    S.ko[j] = kHmacZeroKo[j];
    S.v[j] = 0x01010101u;
  }
  PBFTV_NOUNROLL for (uint32_t sep = 0; sep < 2; ++sep) drbg_passes(S, 0, sep, true, x, h);
  S.fresh = 1;
}

// The next candidate T of step h as LE words; between candidates the
// K = HMAC_K(V || 00), V = HMAC_K(V) update.  The caller keeps the first
// candidate with 0 < k < n.
PBFTV_HD void rfc6979_next(rfc6979_state& S, uint32_t k_words[8]) {
  if (!S.fresh) drbg_passes(S, 0, 0, false, S.v, S.v);  // (x, h unread without data)
  S.fresh = 0;
  drbg_passes(S, 5, 0, false, S.v, S.v);
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) k_words[j] = S.v[7 - j];
}

// r = x mod n for an affine coordinate x < p as LE words (p < 2n)
PBFTV_HD void sign_x_mod_n(uint32_t r[8], const uint32_t x[8]) { words_cond_sub_n(r, x); }

// R = k*G over the width-16 comb, unchecked; false: no digit was non-zero.
//
// For 0 < k < n no addition here is exceptional.  Before window i the sum is
// m*G with m = (k mod 2^(16 i)) - c 2^(16 i), c the recoding carry, so
// |m| <= 2^(16 i - 1), and m = 0 only while every digit so far was zero (the
// `inf` state, a select).  The window adds t*G, t = d_i 2^(16 i) with
// 1 <= |d_i| <= 2^15, so |t| >= 2^(16 i) > |m|: the two points could meet
// only as m == +-t (mod n) with m != +-t.  For i <= 15, |m| + |t| <= 2^255 +
// 2^239 < n rules that out.  The top window (i = 16) holds the carry alone:
// t = 2^256 and m = k - 2^256 in [-2^255, 0).  With q = 2^256 - n (< 2^225),
// m == t means m = q - j n, negative first at j = 1 where it is 2^256 - 2n <
// -2^255; m == -t means m = -q + j n, and the only value in range is -q
// itself (j = 0), which is k = n.  The single Z == 0 test and the exact
// rerun stay anyway (ecdsa_sign_with_k), as in varbase_mult_fast / _exact:
// they cost one canonicalisation, and a table or digit fault then yields a
// correct signature or a refusal, never a wrong point.
template <class LoadG>
PBFTV_HD bool sign_mult_fast(jac& acc, const uint32_t k[8], LoadG ldg) {
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) acc.x.v[l] = acc.y.v[l] = acc.z.v[l] = 0;
  bool inf = true;
  vb_gpart(acc, inf, k, ldg);
  return !inf;
}

// The exact form: every meeting handled (a doubling where two points are
// equal, infinity where they cancel).  Branches on k's digits: it runs only
// where the fast form reported Z == 0, which no 0 < k < n reaches.
template <class LoadG>
PBFTV_HD bool sign_mult_exact(jac& acc, const uint32_t k[8], LoadG ldg) {
  bool inf = true;
  uint32_t w[8];
  PBFTV_UNROLL for (int j = 0; j < 8; ++j) w[j] = k[j];
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

// r = (X / Z^2 mod p) mod n as LE words, R finite
PBFTV_HD void sign_r_from_point(uint32_t r[8], const jac& R) {
  fe zi, zi2, x, one;
  fe_inv(zi, R.z);
  fe_sqr(zi2, zi);
  fe_mul(x, R.x, zi2);
  PBFTV_UNROLL for (int l = 0; l < 9; ++l) one.v[l] = l == 0 ? 1u : 0u;
  fe_mul(x, x, one);  // out of Montgomery form
  fe_canon(x, x);
  uint32_t xw[8];
  fe_to_words(xw, x);
  sign_x_mod_n(r, xw);
}

// s = kinv (e + r d) mod n, all LE words (kinv, r, d canonical; e < 2^256);
// false when s == 0
PBFTV_HD bool sign_s(uint32_t s[8], const uint32_t e[8], const uint32_t d[8], const uint32_t r[8],
                     const uint32_t kinv[8]) {
  fe ef, df, rf, kf, r2n, t, sum;
  fe_from_words(ef, e);
  fe_from_words(df, d);
  fe_from_words(rf, r);
  fe_from_words(kf, kinv);
  fe_set(r2n, kR2N);
  fn_mul(t, rf, r2n);   // r R
  fn_mul(t, t, df);     // r d           (< 2n)
  fe_add(sum, t, ef);   // e + r d, lazy (limbs < 2^30, value < 2^258)
  fn_mul(t, kf, r2n);   // kinv R
  fn_mul(t, t, sum);    // kinv (e + r d)  (< 2n)
  fn_canon(t, t);
  fe_to_words(s, t);
  uint32_t o = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) o |= s[i];
  return o != 0;
}

// One signature under the explicit nonce k (0 < k < n; any other k: false).
// e: the hash as an integer (reduced mod n here), d: the private key, LE
// words.  r_out, s_out: LE words, written only on success.  false when r == 0
// or s == 0.
template <class LoadG>
PBFTV_HD bool ecdsa_sign_with_k(const uint32_t e[8], const uint32_t d[8], const uint32_t k[8], uint32_t r_out[8],
                                uint32_t s_out[8], LoadG ldg, int* out_path = nullptr) {
  if (out_path) *out_path = 0;
  if (!sign_scalar_ok(k)) return false;
  jac R;
  bool fin = sign_mult_fast(R, k, ldg);
  if (fin && fe_is_zero(R.z)) {
    if (out_path) *out_path = 1;
    fin = sign_mult_exact(R, k, ldg);
  }
  if (!fin) return false;
  uint32_t r[8], s[8], kinv[8];
  sign_r_from_point(r, R);
  inv_mod_n_words_ct(kinv, k);
  const bool s_ok = sign_s(s, e, d, r, kinv);
  uint32_t o = 0;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) o |= r[i];
  if (o == 0 || !s_ok) return false;
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) {
    r_out[i] = r[i];
    s_out[i] = s[i];
  }
  return true;
}

// The first usable nonce of (d, h1): candidates until 0 < k < n, at most
// kSignMaxCandidates in all; `from`: how many were taken before this call.
// Returns the index of the candidate kept, or -1.
PBFTV_HD int sign_nonce(rfc6979_state& S, uint32_t k[8], int from) {
  PBFTV_NOUNROLL for (int j = from; j < kSignMaxCandidates; ++j) {
    rfc6979_next(S, k);
    if (sign_scalar_ok(k)) return j;
  }
  return -1;
}

// The whole signature: init, then candidates until ecdsa_sign_with_k
// succeeds, at most kSignMaxCandidates in all.  false (r_out, s_out all
// zero): d out of range or the bound reached.
template <class LoadG>
PBFTV_HD bool ecdsa_sign(const uint32_t e_words[8], const uint32_t d_words[8], uint32_t r_out[8], uint32_t s_out[8],
                         LoadG ldg) {
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) r_out[i] = s_out[i] = 0;
  if (!sign_scalar_ok(d_words)) return false;
  rfc6979_state S;
  rfc6979_init(S, d_words, e_words);
  int j = 0;
  PBFTV_NOUNROLL while (j < kSignMaxCandidates) {
    uint32_t k[8];
    j = sign_nonce(S, k, j);
    if (j < 0) return false;
    if (ecdsa_sign_with_k(e_words, d_words, k, r_out, s_out, ldg)) return true;
    ++j;
  }
  return false;
}

// 32 big-endian bytes -> LE words, LE words -> 32 big-endian bytes (host side
// and the harness; the kernels load and store 16 bytes at a time)
inline void sign_words_from_be(uint32_t w[8], const uint8_t* b) {
  for (int i = 0; i < 8; ++i)
    w[7 - i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}
inline void sign_words_to_be(uint8_t* b, const uint32_t w[8]) {
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) b[4 * i + j] = (uint8_t)(w[7 - i] >> (24 - 8 * j));
}

}  // namespace pbftv
