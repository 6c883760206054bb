// sign_harness.cpp -- TEST INFRASTRUCTURE ONLY.
//
// simple_pbft_amd/csrc/sign.h (deterministic ECDSA-P256 signing: the RFC 6979
// HMAC-DRBG, k*G over the width-16 comb, s = k^-1 (e + r d)) and der.h's
// writer compiled with g++ for tests/test_sign_cpu.py, which compares every
// output byte with tests/rfc6979_model.py.  Built as a shared object for the
// test, and with -DSIGN_MAIN as a stand-alone program (own main, for a
// -fsanitize=address,undefined build) that calls the same entry points on
// heap buffers of exactly the documented sizes and checks them against the two
// P-256 / SHA-256 rows of RFC 6979 §A.2.5.  Never linked into the product
// library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/der.h"
#include "../../simple_pbft_amd/csrc/sign.h"

using namespace pbftv;

namespace {

struct GLoad {
  const uint32_t* gtab;
  void operator()(int win, int idx, uint32_t* out) const {
    memcpy(out, gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 16, 64);
  }
};

}  // namespace

extern "C" {

uint64_t h_sg_g_table_words() { return CombGeom<kVbGBits>::kWords; }

// the width-16 comb table of G (34 MiB), p256_algo.h's serial builder
void h_sg_build_g_table(uint32_t* table) {
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  std::vector<fe> scratch(4 * 256);
  std::vector<uint32_t> lbuf(256 * 16), hbuf(256 * 16);
  build_table_serial<kVbGBits>(table, gx, gy, lbuf.data(), hbuf.data(),
                               [&](int slot, const fe& v) { scratch[slot] = v; },
                               [&](int slot, fe& v) { v = scratch[slot]; });
}

// the first ncand candidates of (d, h1): 32 big-endian bytes each in, ncand * 32 out
void h_sg_drbg(const uint8_t* d_be, const uint8_t* h1_be, int ncand, uint8_t* out) {
  uint32_t d[8], h[8], k[8];
  sign_words_from_be(d, d_be);
  sign_words_from_be(h, h1_be);
  rfc6979_state S;
  rfc6979_init(S, d, h);
  for (int j = 0; j < ncand; ++j) {
    rfc6979_next(S, k);
    sign_words_to_be(out + 32 * j, k);
  }
}

// n rows (e, d, k: 32 B big-endian each) -> r||s (64 B, zeros where refused),
// one ok byte, paths[i] bit 0: the exact rerun ran
void h_sg_sign_with_k(uint64_t n, const uint8_t* e_be, const uint8_t* d_be, const uint8_t* k_be,
                      const uint32_t* gtab, uint8_t* out_rs, uint8_t* out_ok, int* paths) {
  const GLoad ldg{gtab};
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t e[8], d[8], k[8], r[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    sign_words_from_be(e, e_be + 32 * i);
    sign_words_from_be(d, d_be + 32 * i);
    sign_words_from_be(k, k_be + 32 * i);
    int path = 0;
    out_ok[i] = ecdsa_sign_with_k(e, d, k, r, s, ldg, &path) ? 1 : 0;
    sign_words_to_be(out_rs + 64 * i, r);
    sign_words_to_be(out_rs + 64 * i + 32, s);
    if (paths) paths[i] = path;
  }
}

void h_sg_x_mod_n(const uint8_t* x_be, uint8_t* out_be) {
  uint32_t x[8], r[8];
  sign_words_from_be(x, x_be);
  sign_x_mod_n(r, x);
  sign_words_to_be(out_be, r);
}

int h_sg_key_ok(const uint8_t* d_be) {
  uint32_t d[8];
  sign_words_from_be(d, d_be);
  return sign_scalar_ok(d) ? 1 : 0;
}

// n rows (e, d) -> the deterministic signature, as ecdsa_sign computes it
void h_sg_sign(uint64_t n, const uint8_t* e_be, const uint8_t* d_be, const uint32_t* gtab, uint8_t* out_rs,
               uint8_t* out_ok) {
  const GLoad ldg{gtab};
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t e[8], d[8], r[8], s[8];
    sign_words_from_be(e, e_be + 32 * i);
    sign_words_from_be(d, d_be + 32 * i);
    out_ok[i] = ecdsa_sign(e, d, r, s, ldg) ? 1 : 0;
    sign_words_to_be(out_rs + 64 * i, r);
    sign_words_to_be(out_rs + 64 * i + 32, s);
  }
}

// rs: 64 bytes, out: a 72-byte slot (all of it written); the encoding's length
uint32_t h_sg_der_from_rs(const uint8_t* rs, uint8_t* out) { return der_from_rs(rs, out); }

}  // extern "C"

#if defined(SIGN_MAIN)
namespace {

void unhex(const char* s, uint8_t* out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned v = 0;
    sscanf(s + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}

// a heap block of exactly n bytes (so the sanitizer sees any byte past it)
struct Exact {
  uint8_t* p;
  explicit Exact(size_t n) : p((uint8_t*)malloc(n)) { memset(p, 0xA5, n); }
  ~Exact() { free(p); }
};

struct Row {
  const char *hash, *k, *r, *s;
};

}  // namespace

int main() {
  // RFC 6979 §A.2.5, P-256 with SHA-256: the key, then "sample" and "test"
  const char* key = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721";
  const Row rows[2] = {
      {"AF2BDBE1AA9B6EC1E2ADE1D694F41FC71A831D0268E9891562113D8A62ADD1BF",
       "A6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60",
       "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716",
       "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8"},
      {"9F86D081884C7D659A2FEAA0C55AD015A3BF4F1B2B0B822CD15D6C15B0F00A08",
       "D16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0",
       "F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367",
       "019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083"}};
  std::vector<uint32_t> gtab(h_sg_g_table_words());
  h_sg_build_g_table(gtab.data());
  int bad = 0;
  Exact d(32), ds(64), hs(64), ks(64);
  unhex(key, d.p, 32);
  for (int i = 0; i < 2; ++i) {
    memcpy(ds.p + 32 * i, d.p, 32);
    unhex(rows[i].hash, hs.p + 32 * i, 32);
    unhex(rows[i].k, ks.p + 32 * i, 32);
  }
  for (int i = 0; i < 2; ++i) {
    Exact cand(3 * 32), want(32);
    h_sg_drbg(d.p, hs.p + 32 * i, 3, cand.p);
    unhex(rows[i].k, want.p, 32);
    if (memcmp(cand.p, want.p, 32)) {
      fprintf(stderr, "row %d: first candidate differs from the RFC's k\n", i);
      ++bad;
    }
  }
  Exact want_rs(128);
  for (int i = 0; i < 2; ++i) {
    unhex(rows[i].r, want_rs.p + 64 * i, 32);
    unhex(rows[i].s, want_rs.p + 64 * i + 32, 32);
  }
  {
    Exact rs(128), ok(2);
    h_sg_sign_with_k(2, hs.p, ds.p, ks.p, gtab.data(), rs.p, ok.p, nullptr);
    if (memcmp(rs.p, want_rs.p, 128) || ok.p[0] != 1 || ok.p[1] != 1) {
      fprintf(stderr, "sign_with_k differs from the RFC's (r, s)\n");
      ++bad;
    }
  }
  {
    Exact rs(128), ok(2);
    h_sg_sign(2, hs.p, ds.p, gtab.data(), rs.p, ok.p);
    if (memcmp(rs.p, want_rs.p, 128) || ok.p[0] != 1 || ok.p[1] != 1) {
      fprintf(stderr, "sign differs from the RFC's (r, s)\n");
      ++bad;
    }
    // the second row's s starts with a 01 byte, the first row's r and s have
    // their top bits set: 72 and 71 bytes
    for (int i = 0; i < 2; ++i) {
      Exact slot(72), back(64);
      const uint32_t len = h_sg_der_from_rs(rs.p + 64 * i, slot.p);
      uint32_t w[16];
      const bool parsed = der_to_rs_words(DerPtrReader{slot.p}, len, w);
      der_store_rs(w, back.p);
      if (!parsed || memcmp(back.p, rs.p + 64 * i, 64) || len != (i == 0 ? 72u : 71u)) {
        fprintf(stderr, "row %d: DER slot (length %u) does not parse back\n", i, len);
        ++bad;
      }
    }
  }
  {  // DER extremes: the shortest (r = s = 0 -> 8 bytes) and the longest slot, a zero key, x mod n
    Exact rs(64), slot(72);
    memset(rs.p, 0, 64);
    if (h_sg_der_from_rs(rs.p, slot.p) != 8) ++bad;
    memset(rs.p, 0xFF, 64);
    if (h_sg_der_from_rs(rs.p, slot.p) != 72 || slot.p[71] != 0xFF) ++bad;
    Exact z(32), out(32);
    memset(z.p, 0, 32);
    if (h_sg_key_ok(z.p) != 0 || h_sg_key_ok(d.p) != 1) ++bad;
    memset(z.p, 0xFF, 32);
    if (h_sg_key_ok(z.p) != 0) ++bad;
    h_sg_x_mod_n(d.p, out.p);
    if (memcmp(out.p, d.p, 32)) ++bad;
  }
  printf("sign: %d mismatches\n", bad);
  return bad != 0;
}
#endif
