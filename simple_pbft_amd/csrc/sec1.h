// sec1.h -- public keys in SEC1 wire form (SEC1 v2 §2.3.3 / §2.3.4, restricted
// to what go1.19 elliptic.Unmarshal / UnmarshalCompressed accept) for the
// verify under keys that were never registered (varbase.h):
//   kKeyXY                X || Y            64 B  (pub_xy as registration takes it)
//   kKeySec1Compressed    02|03 || X        33 B
//   kKeySec1Uncompressed  04 || X || Y      65 B
// A compressed key costs one square root mod p.  p == 3 (mod 4), so for
// t = X^3 - 3X + b the candidate is y = t^((p+1)/4) and X has a point iff
// y^2 == t (about half of all X have none).  The exponent
//   (p+1)/4 = 2^254 - 2^222 + 2^190 + 2^94 = ((2^32 - 1) 2^128 + 2^96 + 1) 2^94
// is walked by an addition chain: x^(2^32 - 1) from doubling blocks, then
// three runs of squarings -- 253 squarings and 7 products, against fe_pow's
// 256 + 128.  The y of the wanted parity is picked on the canonical value out
// of Montgomery form, as SEC1 states the rule.
//
// Compiled by hipcc for k_varbase_keys_sec1 (p256_varbase.hip) and by g++ for
// the CPU harness (tests/cpp/sec1_harness.cpp), which runs this same limb code.
#pragma once
#include "p256_algo.h"

namespace pbftv {

// the values of PBFTV_KEY_* (include/pbftv.h; pbftv_api.cpp asserts they agree)
constexpr int kKeyXY = 0;
constexpr int kKeySec1Compressed = 1;
constexpr int kKeySec1Uncompressed = 2;

// bytes per key of a format; 0: unknown format
PBFTV_HD uint32_t sec1_key_bytes(int fmt) {
  return fmt == kKeyXY ? 64u : fmt == kKeySec1Compressed ? 33u : fmt == kKeySec1Uncompressed ? 65u : 0u;
}

// n repeated Montgomery squarings mod p (a real loop on the device, as
// fn_sqr_n: one squaring's code, not n of them)
PBFTV_HD void fe_sqr_n(fe& a, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < n; ++i) fe_sqr(a, a);
}

// y = t^((p+1)/4) (Montgomery in, M-type out; t any of M/N/L); true iff
// y^2 == t, that is iff t is a square (0 included: y = 0).
PBFTV_HD bool fe_sqrt_p(fe& y, const fe& t) {
  fe a = t, b;
  fe_sqr_n(a, 1);
  fe_mul(a, a, t);   // t^(2^2 - 1)
  b = a;
  fe_sqr_n(a, 2);
  fe_mul(a, a, b);   // t^(2^4 - 1)
  b = a;
  fe_sqr_n(a, 4);
  fe_mul(a, a, b);   // t^(2^8 - 1)
  b = a;
  fe_sqr_n(a, 8);
  fe_mul(a, a, b);   // t^(2^16 - 1)
  b = a;
  fe_sqr_n(a, 16);
  fe_mul(a, a, b);   // t^(2^32 - 1)
  fe_sqr_n(a, 32);
  fe_mul(a, a, t);   // t^((2^32 - 1) 2^32 + 1)
  fe_sqr_n(a, 96);
  fe_mul(a, a, t);   // t^((2^32 - 1) 2^128 + 2^96 + 1)
  fe_sqr_n(a, 94);   // t^((p + 1) / 4)
  y = a;
  fe_sqr(b, a);
  return fe_equal(b, t);
}

// 32 big-endian bytes (any alignment) -> 8 LE words
PBFTV_HD void sec1_be32_words(uint32_t w[8], const uint8_t* b) {
  PBFTV_UNROLL for (int i = 0; i < 8; ++i) {
    const uint8_t* q = b + 4 * (7 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
}

// A compressed key: prefix (02 / 03) and X as LE words -> the point with
// y == prefix (mod 2); false: X >= p, or X has no point on the curve.
PBFTV_HD bool sec1_decompress(uint32_t prefix, const uint32_t x_w[8], fe& xm, fe& ym) {
  if (!words_lt(x_w, kP32)) return false;
  fe x, r2p, t, u, b, one, yc;
  fe_from_words(x, x_w);
  fe_set(r2p, kR2P);
  fe_mul(xm, x, r2p);
  fe_sqr(t, xm);
  fe_mul(t, t, xm);           // x^3
  fe_mul_small(u, xm, 3);
  fe_sub(t, t, u);            // x^3 - 3x
  fe_set(b, kBMont);
  fe_add(t, t, b);
  if (!fe_sqrt_p(ym, t)) return false;
  PBFTV_UNROLL for (int i = 0; i < 9; ++i) one.v[i] = i == 0 ? 1u : 0u;
  fe_mul(yc, ym, one);        // out of Montgomery form
  fe_canon(yc, yc);           // y in [0, p); y == 0 cannot occur (the group order is odd)
  if (((yc.v[0] ^ prefix) & 1u) != 0) {  // the other root: p - y
    fe_neg_lazy(u, ym);
    fe_norm(ym, u);
  }
  return true;
}

// key_check for a key in wire form (fmt: kKey*; sec1_key_bytes(fmt) bytes at
// key, any alignment): true iff the encoding is accepted and names a point of
// the curve; xm, ym are then its coordinates in Montgomery form.  The hybrid
// forms (06 / 07), the point at infinity (00) and every other first byte are
// rejected.
PBFTV_HD bool sec1_key_check(const uint8_t* key, int fmt, fe& xm, fe& ym) {
  uint32_t xw[8], yw[8];
  if (fmt == kKeySec1Compressed) {
    const uint32_t prefix = key[0];
    if (prefix != 2u && prefix != 3u) return false;
    sec1_be32_words(xw, key + 1);
    return sec1_decompress(prefix, xw, xm, ym);
  }
  if (fmt == kKeySec1Uncompressed) {
    if (key[0] != 4u) return false;
    sec1_be32_words(xw, key + 1);
    sec1_be32_words(yw, key + 33);
    return key_check(xw, yw, xm, ym);
  }
  if (fmt == kKeyXY) {
    sec1_be32_words(xw, key);
    sec1_be32_words(yw, key + 32);
    return key_check(xw, yw, xm, ym);
  }
  return false;
}

}  // namespace pbftv
