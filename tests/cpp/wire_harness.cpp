// wire_harness.cpp -- wire.h (the sealed wire forms' lengths, bounds and
// offsets) and gojson_enc.h's *_signed encoders compiled for the CPU
// (tests/test_wire_cpu.py).  Each h_wire_* call returns wire.h's length from
// the unsigned encoder's preimage length -- what k_seal_lengths computes -- and
// runs the *_signed encoder through a sink bounded by that length, the shape
// of the seal kernels' sink: *overflow counts the bytes that fell past it.
// With -DWIRE_MAIN: a stand-alone program over random messages (run under the
// address and undefined-behaviour sanitizers).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../simple_pbft_amd/csrc/wire.h"

using namespace pbftv;

namespace {

struct CountSink {
  uint64_t n = 0;
  uint8_t scratch[24];
  void put(uint8_t) { ++n; }
  uint8_t* grow(uint32_t k) {
    n += k;
    return scratch;
  }
};

struct BoundedSink {
  uint8_t* p;
  uint64_t n, cap, over;
  uint8_t dump[24];
  void put(uint8_t b) {
    if (n < cap) p[n] = b;
    else ++over;
    ++n;
  }
  uint8_t* grow(uint32_t k) {
    uint8_t* r = n + k <= cap ? p + n : dump;
    if (n + k > cap) over += k;
    n += k;
    return r;
  }
};

}  // namespace

extern "C" {

// out: wire_len bytes at most (cap); returns wire.h's length; *written = what
// the encoder produced, *overflow = bytes past the length, *bound = wire.h's bound
uint64_t h_wire_vote(int64_t view, int64_t seq, const uint8_t* dg, uint64_t dgn, const uint8_t* nid, uint64_t nidn,
                     int64_t mt, const uint8_t* sig, uint64_t sign, uint8_t* out, uint64_t cap, uint64_t* written,
                     uint64_t* overflow, uint64_t* bound) {
  CountSink c;
  gojson::vote(c, view, seq, dg, dgn, nid, nidn, mt);
  const uint64_t len = wire::signed_len(c.n, sign);
  BoundedSink o{out, 0, len < cap ? len : cap, 0, {}};
  gojson::vote_signed(o, view, seq, dg, dgn, nid, nidn, mt, sig, sign, false);
  *written = o.n;
  *overflow = o.over;
  *bound = wire::vote_signed_bound(dgn, nidn, sign);
  return len;
}

uint64_t h_wire_reply(int64_t view, int64_t ts, const uint8_t* cid, uint64_t cidn, const uint8_t* nid, uint64_t nidn,
                      const uint8_t* res, uint64_t resn, const uint8_t* sig, uint64_t sign, uint8_t* out, uint64_t cap,
                      uint64_t* written, uint64_t* overflow, uint64_t* bound) {
  CountSink c;
  gojson::reply(c, view, ts, cid, cidn, nid, nidn, res, resn);
  const uint64_t len = wire::signed_len(c.n, sign);
  BoundedSink o{out, 0, len < cap ? len : cap, 0, {}};
  gojson::reply_signed(o, view, ts, cid, cidn, nid, nidn, res, resn, gojson::SigField{sig, sign, false});
  *written = o.n;
  *overflow = o.over;
  *bound = wire::reply_signed_bound(cidn, nidn, resn, sign);
  return len;
}

uint64_t h_wire_preprepare(int64_t view, int64_t seq, const uint8_t* dg, uint64_t dgn, int has_req, int64_t rts,
                           const uint8_t* rcid, uint64_t rcidn, const uint8_t* rop, uint64_t ropn, int64_t rseq,
                           const uint8_t* rsig, uint64_t rsign, int rsig_nil, const uint8_t* sig, uint64_t sign,
                           uint8_t* out, uint64_t cap, uint64_t* written, uint64_t* overflow, uint64_t* bound) {
  CountSink c;
  gojson::preprepare(c, view, seq, dg, dgn, has_req != 0, rts, rcid, rcidn, rop, ropn, rseq);
  const uint64_t len = wire::preprepare_signed_len(c.n, has_req != 0, rsign, rsig_nil != 0, sign);
  BoundedSink o{out, 0, len < cap ? len : cap, 0, {}};
  gojson::preprepare_signed(o, view, seq, dg, dgn, has_req != 0, rts, rcid, rcidn, rop, ropn, rseq,
                            gojson::SigField{rsig, rsign, rsig_nil != 0}, gojson::SigField{sig, sign, false});
  *written = o.n;
  *overflow = o.over;
  *bound = wire::preprepare_signed_bound(dgn, has_req ? rcidn : 0, has_req ? ropn : 0, rsign, sign);
  return len;
}

uint64_t h_wire_scan(const uint32_t* len, uint64_t n, uint64_t* off) { return wire::scan_offsets(len, n, off); }

uint32_t h_wire_scan_block(void) { return wire::kScanBlock; }
uint32_t h_wire_scan_chunk(void) { return wire::kScanChunk; }

}  // extern "C"

#ifdef WIRE_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// strings out of the escaping families: plain, escapes, controls, HTML,
// U+2028/9, valid multi-byte, invalid and truncated UTF-8, empty
std::vector<uint8_t> rand_str() {
  static const char* parts[] = {"x", "<", ">", "&", "\"", "\\", "\t", "\n", "\x01", "\x7f", "\xe2\x80\xa8",
                                "\xe2\x80\xa9", "\xff", "\xc2\xa2", "\xe0\x9f\xbf", "\xf0\x90\x80\x80",
                                "\xef\xbf\xbd", "\xe2\x82", "\xc0\x80", "abcdef0123456789"};
  std::vector<uint8_t> s;
  for (uint64_t k = rnd() % 9; k-- > 0;)
    for (const char* p = parts[rnd() % (sizeof parts / sizeof *parts)]; *p; ++p) s.push_back((uint8_t)*p);
  return s;
}

int64_t rand_int() {
  static const int64_t ext[] = {0, 1, -1, INT64_MAX, INT64_MIN, 9, 10, -10, 999999999999999999ll};
  return rnd() % 3 ? (int64_t)rnd() >> (rnd() % 64) : ext[rnd() % 9];
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t iters = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  static const uint32_t sig_lens[] = {0, 1, 2, 3, 64, 68, 69, 70, 71, 72, 80};
  uint64_t bad = 0;
  for (uint64_t it = 0; it < iters; ++it) {
    const auto a = rand_str(), b = rand_str(), c = rand_str();
    std::vector<uint8_t> sig(sig_lens[rnd() % 11]), rsig(sig_lens[rnd() % 11]);
    for (auto& x : sig) x = (uint8_t)rnd();
    for (auto& x : rsig) x = (uint8_t)rnd();
    const int64_t v = rand_int(), s = rand_int(), t = rand_int();
    uint64_t wr, ov, bd;
    std::vector<uint8_t> out;
    // exact-size buffers: a byte past the length is a sanitizer report
    uint64_t len = h_wire_vote(v, s, a.data(), a.size(), b.data(), b.size(), t, sig.data(), sig.size(), nullptr, 0,
                               &wr, &ov, &bd);
    out.assign(len, 0);
    h_wire_vote(v, s, a.data(), a.size(), b.data(), b.size(), t, sig.data(), sig.size(), out.data(), len, &wr, &ov,
                &bd);
    bad += wr != len || ov != 0 || bd < len;
    len = h_wire_reply(v, s, a.data(), a.size(), b.data(), b.size(), c.data(), c.size(), sig.data(), sig.size(),
                       nullptr, 0, &wr, &ov, &bd);
    out.assign(len, 0);
    h_wire_reply(v, s, a.data(), a.size(), b.data(), b.size(), c.data(), c.size(), sig.data(), sig.size(), out.data(),
                 len, &wr, &ov, &bd);
    bad += wr != len || ov != 0 || bd < len;
    const int has = rnd() % 4 != 0, rnil = rnd() % 4 == 0;
    len = h_wire_preprepare(v, s, a.data(), a.size(), has, t, b.data(), b.size(), c.data(), c.size(), v,
                            rnil ? nullptr : rsig.data(), rnil ? 0 : rsig.size(), rnil, sig.data(), sig.size(),
                            nullptr, 0, &wr, &ov, &bd);
    out.assign(len, 0);
    h_wire_preprepare(v, s, a.data(), a.size(), has, t, b.data(), b.size(), c.data(), c.size(), v,
                      rnil ? nullptr : rsig.data(), rnil ? 0 : rsig.size(), rnil, sig.data(), sig.size(), out.data(),
                      len, &wr, &ov, &bd);
    bad += wr != len || ov != 0 || bd < len;
  }
  // the scan: zeros, large lengths, a total past 2^32
  std::vector<uint32_t> len(5000);
  for (auto& x : len) x = rnd() % 3 ? (uint32_t)rnd() : 0;
  std::vector<uint64_t> off(len.size());
  const uint64_t total = h_wire_scan(len.data(), len.size(), off.data());
  uint64_t t = 0;
  for (size_t i = 0; i < len.size(); ++i) {
    bad += off[i] != t;
    t += len[i];
  }
  bad += t != total || total <= UINT32_MAX;
  printf("wire: %llu mismatches\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
#endif
