// qc_mail.h on the host for tests/test_qc_mail_cpu.py: the writer posts
// requests into a mailbox that is a heap block of exactly
// QcMail::bytes(kQcCap) bytes, and the reader runs over snapshots built the
// way a wave loads them (lane l reads the dword at qc_poll_off / qc_helper_off).
// Every check returns its number of failures and says each on stderr.  With
// -DQC_MAIL_MAIN it is a stand-alone program (built with
// -fsanitize=address,undefined) that runs all of them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/qc_mail.h"

using namespace pbftv;

namespace {

constexpr uint32_t kSlots = QcMail::kQcSlots, kCap = QcMail::kQcCap;
typedef uint32_t Snap[64];

int fails = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++fails;                      \
      fprintf(stderr, "qc_mail: "); \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
    }                               \
  } while (0)

struct Rng {  // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
};

struct Request {
  uint32_t n;
  std::vector<uint8_t> hashes, sigs;
  std::vector<uint32_t> keys;
  Request(uint32_t n_, Rng& g) : n(n_), hashes(32 * n_), sigs(64 * n_), keys(n_) {
    for (auto& x : hashes) x = (uint8_t)g.next();
    for (auto& x : sigs) x = (uint8_t)g.next();
    for (auto& x : keys) x = g.next();
  }
};

struct Mail {
  uint8_t* p;
  Mail() : p(static_cast<uint8_t*>(calloc(1, QcMail::bytes(kCap)))) {}
  ~Mail() { free(p); }
  void post(const Request& q, uint32_t cur) {  // as the host does: the helpers' inputs, then the slots and the bell
    if (q.n > kSlots) qc_write_arrays(p, kCap, q.hashes.data(), q.sigs.data(), q.keys.data(), kSlots, q.n);
    qc_post(p, cur, q.n, q.hashes.data(), q.sigs.data(), q.keys.data());
  }
  QcMail* hdr() { return reinterpret_cast<QcMail*>(p); }
  // slot b's poll, as its wave loads it
  void poll(uint32_t b, Snap v) const {
    for (uint32_t l = 0; l < 64; ++l) memcpy(&v[l], p + qc_poll_off(b, l), 4);
  }
  void helper(uint32_t b, Snap v) const {
    for (uint32_t l = 0; l < 64; ++l) memcpy(&v[l], p + qc_helper_off(b, l), 4);
  }
};

// 32 big-endian bytes as the kernels' little-endian words, byte by byte
bool same_be256(const uint32_t w[8], const uint8_t* be) {
  for (int j = 0; j < 8; ++j) {
    const uint8_t* q = be + 28 - 4 * j;
    if (w[j] != (((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3])) return false;
  }
  return true;
}
bool decoded_is(const Request& q, uint32_t i, const uint32_t e[8], const uint32_t r[8], const uint32_t s[8], uint32_t key) {
  return same_be256(e, &q.hashes[32 * i]) && same_be256(r, &q.sigs[64 * i]) && same_be256(s, &q.sigs[64 * i + 32]) &&
         key == q.keys[i];
}

}  // namespace

extern "C" {

uint64_t h_qc_mail_bytes() { return QcMail::bytes(kCap); }

// request cur of n signatures over a complete request cur - 1 of n_old
int h_qc_check_post(uint32_t n, uint32_t n_old, uint32_t cur, uint64_t seed) {
  fails = 0;
  Rng g{seed | 1};
  Mail m;
  const Request old(n_old, g), q(n, g);
  m.post(old, cur - 1);
  m.post(q, cur);
  CHECK(m.hdr()->bell == cur, "n=%u: bell %u", n, m.hdr()->bell);
  {  // the bytes themselves, once: slot 0 is {tag, n, key, 0, hash, 0, 0, 0, tag}, {tag, 0, 0, 0, r, ...}, {.. s ..}
    uint32_t raw[48] = {};
    for (int line = 0; line < 3; ++line) raw[16 * line] = raw[16 * line + 15] = cur;
    raw[1] = n, raw[2] = q.keys[0];
    memcpy(raw + 4, &q.hashes[0], 32);
    memcpy(raw + 20, &q.sigs[0], 32);
    memcpy(raw + 36, &q.sigs[32], 32);
    CHECK(memcmp(raw, m.p + 64, sizeof raw) == 0, "n=%u: slot 0's bytes", n);
  }
  for (uint32_t b = 0; b < kSlots; ++b) {
    Snap v;
    m.poll(b, v);
    CHECK(qc_slot_ready(v, b, cur), "n=%u slot %u: not ready for the posted request", n, b);
    CHECK(!qc_slot_ready(v, b, cur + 1) && !qc_slot_ready(v, b, cur - 1), "n=%u slot %u: ready for another request", n, b);
    CHECK(qc_slot_n(v) == n, "n=%u slot %u: n read as %u", n, b, qc_slot_n(v));
    CHECK(!qc_cancelled(v, cur, m.hdr()->halt), "n=%u slot %u: cancelled", n, b);
    if (b >= n) {  // ready from line 0 alone: lines 1 and 2 still hold the old request
      CHECK(qc_line_is(v, 0, cur) && !qc_line_is(v, 1, cur) && !qc_line_is(v, 2, cur), "n=%u slot %u: lines past n", n, b);
      continue;
    }
    uint32_t e[8], r[8], s[8], key;
    qc_slot_decode(v, e, r, s, key);
    CHECK(decoded_is(q, b, e, r, s, key), "n=%u slot %u: decode differs from the posted inputs", n, b);
  }
  for (uint32_t b = kSlots; b < n; ++b) {
    Snap v;
    m.helper(b, v);
    uint32_t e[8], r[8], s[8], key;
    qc_helper_decode(v, e, r, s, key);
    CHECK(decoded_is(q, b, e, r, s, key), "n=%u helper %u: decode differs from the posted inputs", n, b);
  }
  return fails;
}

// Every slot, every subset of its three lines from request cur and the rest
// from cur - 1: ready exactly when the lines the slot needs are all new.  And
// a line with one new and one old tag, among otherwise new lines, is never new.
int h_qc_check_tearing(uint32_t n, uint32_t n_old, uint32_t cur, uint64_t seed) {
  fails = 0;
  Rng g{seed | 1};
  Mail before, after;
  const Request old(n_old, g), q(n, g);
  before.post(old, cur - 1);
  after.post(old, cur - 1);
  after.post(q, cur);
  for (uint32_t b = 0; b < kSlots; ++b) {
    Snap vo, vn;
    before.poll(b, vo);
    after.poll(b, vn);
    for (uint32_t mask = 0; mask < 8; ++mask) {
      Snap v;
      memcpy(v, vn, sizeof v);
      for (int line = 0; line < kQcSlotLines; ++line)
        if (!(mask >> line & 1)) memcpy(v + line * kQcLineDwords, vo + line * kQcLineDwords, 4 * kQcLineDwords);
      const bool need = b < n ? mask == 7 : (mask & 1) != 0;
      CHECK(qc_slot_ready(v, b, cur) == need, "n=%u slot %u lines %u: ready %d", n, b, mask, (int)!need);
    }
    for (int line = 0; line < kQcSlotLines; ++line)
      for (int tag : {kQcTagFirst, kQcTagLast}) {
        Snap v;
        memcpy(v, vn, sizeof v);
        v[line * kQcLineDwords + tag] = cur;  // (a slot past n: its lines 1 and 2 are old)
        v[line * kQcLineDwords + (kQcLineDwords - 1 - tag)] = cur - 1;
        CHECK(!qc_line_is(v, line, cur), "n=%u slot %u line %d: new with only tag %d new", n, b, line, tag);
        if (line == 0 || b < n) CHECK(!qc_slot_ready(v, b, cur), "n=%u slot %u line %d: ready with only tag %d new", n, b, line, tag);
      }
  }
  return fails;
}

int h_qc_check_cancel(uint32_t cur, uint64_t seed) {
  fails = 0;
  Rng g{seed | 1};
  Mail m;
  m.post(Request(3, g), cur - 1);
  const uint32_t halt = m.hdr()->halt = g.next();
  for (uint32_t b = 0; b < kSlots; ++b) {
    Snap v;
    m.hdr()->stop = cur - 1;
    m.poll(b, v);
    CHECK(!qc_cancelled(v, cur, halt), "slot %u: cancelled with stop and halt unchanged", b);
    m.hdr()->stop = cur;
    m.poll(b, v);
    CHECK(qc_cancelled(v, cur, halt), "slot %u: stop == want does not cancel", b);
    m.hdr()->stop = cur - 1;
    m.hdr()->halt = halt + 1;
    m.poll(b, v);
    CHECK(qc_cancelled(v, cur, halt), "slot %u: a changed halt does not cancel", b);
    m.hdr()->halt = halt;
  }
  return fails;
}

int h_qc_check_relay() {
  fails = 0;
  const uint32_t vals[] = {0u, 1u, 8u, 9u, 67u, 128u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t number : vals)
    for (uint32_t n : vals) {
      const uint64_t r = qc_relay_pack(number, n);
      CHECK(qc_relay_number(r) == number && qc_relay_n(r) == n, "relay {%u, %u} unpacks as {%u, %u}", number, n,
            qc_relay_number(r), qc_relay_n(r));
      CHECK((qc_relay_n(r) == kQcRelayLeft) == (n == 0xFFFFFFFFu), "relay {%u, %u}: left", number, n);
    }
  CHECK(qc_relay_number(0) == 0 && qc_relay_n(0) == 0, "the zeroed relay");
  return fails;
}

}  // extern "C"

#ifdef QC_MAIL_MAIN
int main() {
  int bad = 0, checks = 0;
  for (uint32_t cur : {2u, 0x80000000u, 0xFFFFFFFEu})
    for (uint32_t n : {1u, 3u, 8u, 9u, 67u, 128u})
      for (uint32_t n_old : {128u, 3u}) {
        bad += h_qc_check_post(n, n_old, cur, 0x51C0FFEEull + n);
        bad += h_qc_check_tearing(n, n_old, cur, 0x7EA2ull + n);
        checks += 2;
      }
  bad += h_qc_check_cancel(7, 11) + h_qc_check_relay();
  checks += 2;
  printf("qc_mail: %d failures over %d checks\n", bad, checks);
  return bad ? 1 : 0;
}
#endif
