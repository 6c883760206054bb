// varbase_harness.cpp -- TEST INFRASTRUCTURE ONLY.
//
// simple_pbft_amd/csrc/varbase.h (verification under a key carried with the
// signature: 4-bit fixed-window ladder over the lane's own key, then the
// width-16 G comb) compiled with g++ for tests/test_varbase_cpu.py, which
// checks varbase_verify_sig bit for bit against the oracle.  Built as a shared
// object for the test, and with -DVARBASE_MAIN as a stand-alone program (own
// main, for a -fsanitize=address,undefined build) that checks the ladder and
// the exact rerun against the G comb alone on edge scalars and a random
// stream, and -- given a dump of tests/carried_cases.py's combined set as its
// second argument -- walks that set through h_vb_verify_batch against the
// recorded bits.  Never linked into the product library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/varbase.h"
#if defined(VARBASE_MAIN)
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

struct GLoad {
  const uint32_t* gtab;
  void operator()(int win, int idx, uint32_t* out) const {
    memcpy(out, gtab + (CombGeom<kVbGBits>::base(win) + (uint64_t)idx) * 16, 64);
  }
};

}  // namespace

extern "C" {

uint64_t h_vb_g_table_words() { return CombGeom<kVbGBits>::kWords; }

// the width-16 comb table of G (34 MiB), p256_algo.h's serial builder
void h_vb_build_g_table(uint32_t* table) {
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  std::vector<fe> scratch(4 * 256);
  std::vector<uint32_t> lbuf(256 * 16), hbuf(256 * 16);
  build_table_serial<kVbGBits>(table, gx, gy, lbuf.data(), hbuf.data(),
                               [&](int slot, const fe& v) { scratch[slot] = v; },
                               [&](int slot, fe& v) { v = scratch[slot]; });
}

// the 65 ladder digits of u (LE words), lowest first
void h_vb_digits(const uint32_t* u, int* out) {
  uint32_t t[8];
  out[kVbWin - 1] = (int)vb_recode(t, u);
  for (int i = kVbWin - 2; i >= 0; --i) out[i] = vb_next_digit(t);
}

// the 17 comb digits of u as the G part cuts them, and as signed_digit_w<16> does
void h_vb_gdigits(const uint32_t* u, int* out, int* out_ref) {
  uint32_t w[8];
  memcpy(w, u, 32);
  int c = 0, c2 = 0;
  for (int i = 0; i < kVbGWin; ++i) {
    out[i] = vb_next_gdigit(w, c);
    out_ref[i] = signed_digit_w<kVbGBits>(u, i, c2);
  }
}

// n signatures (hash 32 B, r||s 64 B, X||Y 64 B, all big-endian) -> one accept
// byte each; paths[i] bit 0: the exact rerun ran
void h_vb_verify_batch(uint64_t n, const uint8_t* hashes, const uint8_t* sigs, const uint8_t* pubs,
                       const uint32_t* gtab, uint8_t* out, int* paths) {
  const GLoad ldg{gtab};
  jac tab[kVbEnt];
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t e[8], r[8], s[8], x[8], y[8];
    be32_to_le_words(hashes + 32 * i, e);
    be32_to_le_words(sigs + 64 * i, r);
    be32_to_le_words(sigs + 64 * i + 32, s);
    be32_to_le_words(pubs + 64 * i, x);
    be32_to_le_words(pubs + 64 * i + 32, y);
    int path = 0;
    out[i] = varbase_verify_sig(e, r, s, x, y, tab, ldg, &path) ? 1 : 0;
    if (paths) paths[i] = path;
  }
}

// chosen scalars (LE words) under the key Q = G against r; *path as above
int h_vb_verify_u(const uint32_t* u1, const uint32_t* u2, const uint32_t* r, const uint32_t* gtab, int* path) {
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  jac tab[kVbEnt];
  return varbase_verify(u1, u2, r, gx, gy, tab, GLoad{gtab}, path) ? 1 : 0;
}

}  // extern "C"

#if defined(VARBASE_MAIN)
namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd32() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// (a + b) mod n on LE words, a, b < n
void add_mod_n(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t cy = 0;
  uint32_t s[8];
  for (int i = 0; i < 8; ++i) {
    cy += (uint64_t)a[i] + b[i];
    s[i] = (uint32_t)cy;
    cy >>= 32;
  }
  if (cy || !words_lt(s, kN32)) {
    int64_t br = 0;
    for (int i = 0; i < 8; ++i) {
      br += (int64_t)s[i] - kN32[i];
      s[i] = (uint32_t)br;
      br >>= 32;
    }
  }
  memcpy(out, s, 32);
}

void sub_n(uint32_t out[8], const uint32_t k[8]) {  // n - k
  int64_t br = 0;
  for (int i = 0; i < 8; ++i) {
    br += (int64_t)kN32[i] - k[i];
    out[i] = (uint32_t)br;
    br >>= 32;
  }
}

// same point? (both finite) X1 Z2^2 == X2 Z1^2 and Y1 Z2^3 == Y2 Z1^3
bool same_point(const jac& a, const jac& b) {
  fe za, zb, l, r, t;
  fe_sqr(za, a.z);
  fe_sqr(zb, b.z);
  fe_mul(l, a.x, zb);
  fe_mul(r, b.x, za);
  if (!fe_equal(l, r)) return false;
  fe_mul(t, za, a.z);
  fe_mul(za, zb, b.z);
  fe_mul(l, a.y, za);
  fe_mul(r, b.y, t);
  return fe_equal(l, r);
}

// u1 G + u2 G by the fast form (and the exact rerun when it asks) against
// (u1 + u2) G by the checked G comb alone; want_rerun < 0: either
int check(const uint32_t* gtab, const uint32_t u1[8], const uint32_t u2[8], int want_rerun, const char* what) {
  const GLoad ldg{gtab};
  fe gx, gy;
  fe_set(gx, kGxMont);
  fe_set(gy, kGyMont);
  jac tab[kVbEnt];
  vb_build_table(gx, gy, [&](int k, const jac& p) { tab[k] = p; });
  auto ld = [&](int idx, jac& p) { p = tab[idx]; };
  jac R, E, S;
  int fin = varbase_mult_fast(R, u1, u2, ld, ldg);
  const int rerun = fin < 0;
  const bool efin = varbase_mult_exact(E, u1, u2, ld, ldg);
  if (rerun) {
    R = E;
    fin = efin ? 1 : 0;
  }
  uint32_t sum[8];
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  add_mod_n(sum, u1, u2);
  bool sinf = true;
  {  // the G comb alone, checked additions
    uint32_t w[8];
    memcpy(w, sum, 32);
    int c = 0;
    for (int i = 0; i < kVbGWin; ++i) {
      const int g = vb_next_gdigit(w, c);
      if (g == 0) continue;
      uint32_t ew[16];
      ldg(i, (g < 0 ? -g : g) - 1, ew);
      comb_add_entry<true>(S, sinf, g, ew);
    }
  }
  (void)zero;
  int bad = 0;
  if ((fin == 1) != !sinf || efin != !sinf) bad = 1;
  else if (!sinf && (!same_point(R, S) || !same_point(E, S))) bad = 1;
  if (want_rerun >= 0 && rerun != want_rerun) bad = 1;
  if (bad) fprintf(stderr, "mismatch: %s (fin %d, exact %d, comb %d, rerun %d)\n", what, fin, (int)efin, (int)!sinf, rerun);
  return bad;
}

void small(uint32_t out[8], uint64_t v, int shift_words = 0) {
  memset(out, 0, 32);
  out[shift_words] = (uint32_t)v;
  if (shift_words + 1 < 8) out[shift_words + 1] = (uint32_t)(v >> 32);
}

}  // namespace

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? atoi(argv[1]) : 64;
  std::vector<uint32_t> gtab(CombGeom<kVbGBits>::kWords);
  h_vb_build_g_table(gtab.data());
  int bad = 0;
  uint32_t u1[8], u2[8], t[8];
  // ladder edges: small u2, nibble boundaries, the top of the range
  const uint64_t edges[] = {1, 2, 7, 8, 9, 15, 16, 17, 0x88, 0x99, 0xFFFF, 0x10000};
  for (uint64_t e : edges) {
    small(u1, 0x1234567);
    small(u2, e);
    bad += check(gtab.data(), u1, u2, -1, "small u2");
  }
  for (int k = 1; k <= 16; ++k) {  // u2 = n - k (n - 2: the ladder's one doubling)
    small(t, (uint64_t)k);
    sub_n(u2, t);
    small(u1, 0x1234567);
    bad += check(gtab.data(), u1, u2, k == 2 ? 1 : -1, "u2 = n - k");
  }
  memset(u2, 0x88, 32);
  small(u1, 3);
  bad += check(gtab.data(), u1, u2, -1, "u2 = 0x88..8");
  memset(u2, 0x99, 32);
  bad += check(gtab.data(), u1, u2, -1, "u2 = 0x99..9");
  // G-part meetings: u1 = u2 = m 2^(16 i) (a doubling at window i)
  for (int w : {0, 4, 7}) {
    small(u1, 77, w);
    small(u2, 77, w);
    bad += check(gtab.data(), u1, u2, 1, "doubling in the G part");
  }
  // final cancellation: (u1, n - u1)
  small(u1, 0xABCDEF, 2);
  sub_n(u2, u1);
  bad += check(gtab.data(), u1, u2, 1, "cancellation at the end");
  // mid-sum cancellation that continues from infinity
  small(u1, 5 + (9ull << 16));
  u1[1] = 3;  // + 3 * 2^32
  small(t, 5 + (9ull << 16));
  sub_n(u2, t);
  bad += check(gtab.data(), u1, u2, 1, "cancellation in the middle");
  for (int it = 0; it < n_random; ++it) {
    for (int i = 0; i < 8; ++i) {
      u1[i] = rnd32();
      u2[i] = rnd32();
    }
    u1[7] &= 0x7FFFFFFFu;  // < n
    u2[7] &= 0x7FFFFFFFu;
    u2[0] |= 1u;
    bad += check(gtab.data(), u1, u2, 0, "random");
  }
  printf("varbase: %d mismatches\n", bad);
  if (argc > 2) {  // the carried-key set: accept bits, and the rerun bit where it is pinned
    CarriedDump d;
    if (!d.read(argv[2])) {
      fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    std::vector<uint8_t> out(d.n);
    std::vector<int> paths(d.n);
    h_vb_verify_batch(d.n, d.hashes.data(), d.sigs.data(), d.xy.data(), gtab.data(), out.data(), paths.data());
    int wrong = 0, reruns = 0;
    for (uint64_t i = 0; i < d.n; ++i) {
      reruns += paths[i] & 1;
      if (out[i] != d.want_xy[i] || (d.rerun[i] != 255 && (paths[i] & 1) != d.rerun[i])) {
        ++wrong;
        fprintf(stderr, "carried mismatch: row %llu (bit %d, rerun %d)\n", (unsigned long long)i, out[i], paths[i] & 1);
      }
    }
    printf("carried: %d mismatches of %llu (%d reruns)\n", wrong, (unsigned long long)d.n, reruns);
    bad += wrong;
  }
  return bad != 0;
}
#endif
