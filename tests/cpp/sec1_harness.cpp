// sec1_harness.cpp -- TEST INFRASTRUCTURE ONLY.
//
// simple_pbft_amd/csrc/sec1.h (public keys in SEC1 wire form: the square root
// mod p by an addition chain, the decode of compressed and uncompressed keys)
// compiled with g++ for tests/test_sec1_cpu.py, which checks fe_sqrt_p and
// sec1_key_check against Python big integers and runs the decoded keys through
// varbase.h's verify against the oracle.  Built as a shared object for the
// test, and with -DSEC1_MAIN as a stand-alone program (own main, for a
// -fsanitize=address,undefined build) that decodes every multiple k G,
// k = 1..64, in both formats and both parities, and a stream of random X, and
// -- given a dump of tests/carried_cases.py's combined set as its second
// argument -- decodes and verifies that set's compressed keys against the
// recorded values.  Never linked into the product library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/sec1.h"
#include "../../simple_pbft_amd/csrc/varbase.h"
#if defined(SEC1_MAIN)
#include "carried_dump.h"
#endif

using namespace pbftv;

namespace {

void be32_to_le_words(const uint8_t* b, uint32_t* w) {
  for (int i = 0; i < 8; ++i) {
    const uint8_t* p = b + 4 * (7 - i);
    w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
  }
}

void le_words_to_be32(const uint32_t* w, uint8_t* b) {
  for (int i = 0; i < 8; ++i) {
    uint8_t* p = b + 4 * (7 - i);
    p[0] = (uint8_t)(w[i] >> 24);
    p[1] = (uint8_t)(w[i] >> 16);
    p[2] = (uint8_t)(w[i] >> 8);
    p[3] = (uint8_t)w[i];
  }
}

// plain value (LE words, < 2^256) -> Montgomery form
void to_mont(fe& m, const uint32_t w[8]) {
  fe a, r2p;
  fe_from_words(a, w);
  fe_set(r2p, kR2P);
  fe_mul(m, a, r2p);
}

// Montgomery form -> canonical 32 big-endian bytes
void from_mont_be(uint8_t out[32], const fe& m) {
  fe one, c;
  for (int i = 0; i < 9; ++i) one.v[i] = i == 0 ? 1u : 0u;
  fe_mul(c, m, one);
  fe_canon(c, c);
  uint32_t w[8];
  fe_to_words(w, c);
  le_words_to_be32(w, out);
}

struct GLoad {
  const uint32_t* gtab;
  void operator()(int win, int idx, uint32_t* out) const {
    memcpy(out, gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 16, 64);
  }
};

}  // namespace

extern "C" {

uint32_t h_sec1_key_bytes(int fmt) { return sec1_key_bytes(fmt); }

// n values t (32 B big-endian each, < 2^256): ok[i] = fe_sqrt_p's verdict,
// y[i] = its y (canonical, big-endian) whether or not it is a root
void h_sec1_sqrt(uint64_t n, const uint8_t* t_be, uint8_t* y_be, uint8_t* ok) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t w[8];
    be32_to_le_words(t_be + 32 * i, w);
    fe t, y;
    to_mont(t, w);
    ok[i] = fe_sqrt_p(y, t) ? 1 : 0;
    from_mont_be(y_be + 32 * i, y);
  }
}

// n keys packed at the format's stride: ok[i] = sec1_key_check's verdict,
// xy[64 i ..] = the decoded point (X||Y canonical big-endian; zeros if rejected)
void h_sec1_decode(uint64_t n, const uint8_t* keys, int fmt, uint8_t* xy, uint8_t* ok) {
  const uint32_t stride = sec1_key_bytes(fmt);
  for (uint64_t i = 0; i < n; ++i) {
    fe xm, ym;
    ok[i] = sec1_key_check(keys + (uint64_t)stride * i, fmt, xm, ym) ? 1 : 0;
    memset(xy + 64 * i, 0, 64);
    if (ok[i]) {
      from_mont_be(xy + 64 * i, xm);
      from_mont_be(xy + 64 * i + 32, ym);
    }
  }
}

uint64_t h_sec1_g_table_words() { return CombGeom<kVbGBits>::kWords; }

void h_sec1_build_g_table(uint32_t* table) {
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  std::vector<fe> scratch(4 * 256);
  std::vector<uint32_t> lbuf(256 * 16), hbuf(256 * 16);
  build_table_serial<kVbGBits>(table, gx, gy, lbuf.data(), hbuf.data(),
                               [&](int slot, const fe& v) { scratch[slot] = v; },
                               [&](int slot, fe& v) { v = scratch[slot]; });
}

// n signatures (hash 32 B, r||s 64 B big-endian, key in fmt at its stride):
// sec1_key_check, stage 1, varbase_verify -> one accept byte each
void h_sec1_verify_batch(uint64_t n, const uint8_t* hashes, const uint8_t* sigs, const uint8_t* keys, int fmt,
                         const uint32_t* gtab, uint8_t* out) {
  const GLoad ldg{gtab};
  const uint32_t stride = sec1_key_bytes(fmt);
  jac tab[kVbEnt];
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t e[8], r[8], s[8], u1[8], u2[8];
    be32_to_le_words(hashes + 32 * i, e);
    be32_to_le_words(sigs + 64 * i, r);
    be32_to_le_words(sigs + 64 * i + 32, s);
    fe xm, ym;
    out[i] = 0;
    if (!sec1_key_check(keys + (uint64_t)stride * i, fmt, xm, ym)) continue;
    if (!ecdsa_scalars(e, r, s, u1, u2)) continue;
    out[i] = varbase_verify(u1, u2, r, xm, ym, tab, ldg) ? 1 : 0;
  }
}

}  // extern "C"

#if defined(SEC1_MAIN)
namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd32() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// affine (X||Y big-endian) of a finite Jacobian point
void affine_be(uint8_t out[64], const jac& p) {
  fe zi;
  fe_inv(zi, p.z);
  uint32_t w[16];
  jac_to_affine_words(w, p, zi);  // Montgomery form, canonical
  fe x, y;
  entry_to_fe(x, y, w);
  from_mont_be(out, x);
  from_mont_be(out + 32, y);
}

// a point in both SEC1 forms and with the other parity: every decode must
// give back (x, y), respectively (x, p - y)
int check_point(const uint8_t xy[64], const char* what) {
  int bad = 0;
  uint8_t c[33], u[65], got[64], ok = 0;
  c[0] = (uint8_t)(2 + (xy[63] & 1));
  memcpy(c + 1, xy, 32);
  u[0] = 4;
  memcpy(u + 1, xy, 64);
  h_sec1_decode(1, c, kKeySec1Compressed, got, &ok);
  if (!ok || memcmp(got, xy, 64)) bad = 1;
  h_sec1_decode(1, u, kKeySec1Uncompressed, got, &ok);
  if (!ok || memcmp(got, xy, 64)) bad = 1;
  h_sec1_decode(1, xy, kKeyXY, got, &ok);
  if (!ok || memcmp(got, xy, 64)) bad = 1;
  c[0] ^= 1;  // the other root: same x, another y, still on the curve
  h_sec1_decode(1, c, kKeySec1Compressed, got, &ok);
  if (!ok || memcmp(got, xy, 32) || !memcmp(got + 32, xy + 32, 32) || (got[63] & 1) != (c[0] & 1)) bad = 1;
  memcpy(u + 1, got, 64);
  uint8_t got2[64];
  h_sec1_decode(1, u, kKeySec1Uncompressed, got2, &ok);
  if (!ok || memcmp(got2, got, 64)) bad = 1;
  for (uint8_t pre : {0, 1, 4, 5, 6, 7, 255}) {
    c[0] = pre;
    h_sec1_decode(1, c, kKeySec1Compressed, got, &ok);
    if (ok) bad = 1;
  }
  for (uint8_t pre : {0, 2, 3, 6, 7}) {
    u[0] = pre;
    h_sec1_decode(1, u, kKeySec1Uncompressed, got, &ok);
    if (ok) bad = 1;
  }
  if (bad) fprintf(stderr, "mismatch: %s\n", what);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 256;
  int bad = 0;
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  jac cur;
  cur.x = gx;
  cur.y = gy;
  fe_set(cur.z, kOneP);
  for (int k = 1; k <= 64; ++k) {  // k G
    if (k == 2) jac_double(cur, cur);
    else if (k > 2) jac_madd<false>(cur, gx, gy);
    uint8_t xy[64];
    affine_be(xy, cur);
    bad += check_point(xy, "k G");
  }
  // random X: either no point (both prefixes rejected), or two points that
  // are each other's negatives and pass the uncompressed check
  int with = 0, without = 0;
  for (int it = 0; it < n_random; ++it) {
    uint8_t c[33], a[64], b[64], oka = 0, okb = 0;
    for (int i = 0; i < 8; ++i) {
      const uint32_t v = rnd32();
      memcpy(c + 1 + 4 * i, &v, 4);
    }
    c[0] = 2;
    h_sec1_decode(1, c, kKeySec1Compressed, a, &oka);
    c[0] = 3;
    h_sec1_decode(1, c, kKeySec1Compressed, b, &okb);
    if (oka != okb) {
      ++bad;
      fprintf(stderr, "mismatch: random X, the prefixes disagree\n");
    } else if (oka) {
      ++with;
      if ((a[63] & 1) != 0 || (b[63] & 1) != 1 || memcmp(a, b, 32)) ++bad;
      bad += check_point(a, "random X");
    } else {
      ++without;
    }
  }
  if (n_random >= 64 && (with == 0 || without == 0)) ++bad;
  printf("sec1: %d mismatches (%d X with a point, %d without)\n", bad, with, without);
  if (argc > 2) {  // the carried-key set under its compressed keys: the decode, then the verify
    CarriedDump d;
    if (!d.read(argv[2])) {
      fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    std::vector<uint8_t> xy(64 * d.n), ok(d.n), out(d.n);
    h_sec1_decode(d.n, d.comp.data(), kKeySec1Compressed, xy.data(), ok.data());
    std::vector<uint32_t> gtab(h_sec1_g_table_words());
    h_sec1_build_g_table(gtab.data());
    h_sec1_verify_batch(d.n, d.hashes.data(), d.sigs.data(), d.comp.data(), kKeySec1Compressed, gtab.data(), out.data());
    int wrong = 0, rejected = 0;
    for (uint64_t i = 0; i < d.n; ++i) {
      rejected += !ok[i];
      if (ok[i] != d.comp_ok[i] || memcmp(&xy[64 * i], &d.comp_xy[64 * i], 64) || out[i] != d.want_comp[i]) {
        ++wrong;
        fprintf(stderr, "carried mismatch: row %llu (key %d, bit %d)\n", (unsigned long long)i, ok[i], out[i]);
      }
    }
    printf("carried: %d mismatches of %llu (%d keys rejected)\n", wrong, (unsigned long long)d.n, rejected);
    bad += wrong;
  }
  return bad != 0;
}
#endif
