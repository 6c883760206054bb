// der_harness.cpp -- simple_pbft_amd/csrc/der.h compiled for the host
// (tests/test_der_cpu.py): the parser k_der_to_rs runs, behind three readers --
//   h_der_ptr      DerPtrReader, what der.cpp uses;
//   h_der_probe    a reader that records the largest index asked for and
//                  answers nothing at or past min(len, 72);
//   h_der_dwords   DerDwordReader, the kernel's reader, over a fetch that
//                  checks every dword it is asked for against the kernel's
//                  read rule (it must hold one of the first min(len, 72) bytes
//                  of the encoding) and poisons the bytes outside the buffer.
// With -DDER_MAIN: a stand-alone program for the sanitizers; it reads a corpus
// file, gives each encoding an exactly-sized heap block and parses it there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/der.h"

namespace {

using namespace pbftv;

struct ProbeReader {
  const uint8_t* p;
  uint32_t limit;          // min(len, 72)
  int64_t* max_index;      // largest index asked for
  uint32_t get(int64_t i) const {
    if (i > *max_index) *max_index = i;
    return i >= 0 && i < (int64_t)limit ? p[i] : 0u;
  }
  uint32_t byte(uint32_t i) const { return get(i); }
  uint32_t tail_word(int32_t i, uint32_t lo) const {
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j)
      if (i + j >= (int32_t)lo) w |= get(i + j) << (8 * j);
    return w;
  }
};

// the data buffer stands at a 4-byte-aligned address; the encoding begins at
// byte `start` of it
struct CheckedFetch {
  const uint8_t* data;
  uint64_t data_bytes, start, limit;  // limit = min(len, 72)
  uint64_t* bad;                      // dwords fetched against the rule
  uint32_t operator()(uint32_t k) const {
    const uint64_t a = (start & ~(uint64_t)3) + 4 * (uint64_t)k;  // first byte of the dword
    if (!(a + 4 > start && a < start + limit)) ++*bad;
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) w |= (uint32_t)(a + j < data_bytes ? data[a + j] : 0xA5u) << (8 * j);
    return w;
  }
};

template <class R>
uint8_t run(const R& rd, uint64_t len, uint8_t* out_rs) {
  uint32_t rs[16];
  const bool ok = der_to_rs_words(rd, len, rs);
  der_store_rs(rs, out_rs);
  return ok ? 1 : 0;
}

}  // namespace

extern "C" {

void h_der_ptr(uint64_t n, const uint8_t* data, const uint64_t* off, const uint32_t* len, uint8_t* out_rs,
               uint8_t* parsed) {
  for (uint64_t i = 0; i < n; ++i)
    parsed[i] = run(DerPtrReader{len[i] ? data + off[i] : nullptr}, len[i], out_rs + 64 * i);
}

// max_index[i]: the largest index the parser asked its reader for (-1: none)
void h_der_probe(uint64_t n, const uint8_t* data, const uint64_t* off, const uint32_t* len, uint8_t* out_rs,
                 uint8_t* parsed, int64_t* max_index) {
  for (uint64_t i = 0; i < n; ++i) {
    max_index[i] = -1;
    const uint32_t limit = len[i] < kDerMaxBytes ? len[i] : kDerMaxBytes;
    parsed[i] = run(ProbeReader{len[i] ? data + off[i] : nullptr, limit, max_index + i}, len[i], out_rs + 64 * i);
  }
}

// returns the number of dwords fetched against the read rule
uint64_t h_der_dwords(uint64_t n, const uint8_t* data, uint64_t data_bytes, const uint64_t* off, const uint32_t* len,
                      uint8_t* out_rs, uint8_t* parsed) {
  uint64_t bad = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (len[i] == 0) {  // (as the kernel: the offset is not looked at)
      std::memset(out_rs + 64 * i, 0, 64);
      parsed[i] = 0;
      continue;
    }
    const uint64_t limit = len[i] < kDerMaxBytes ? len[i] : kDerMaxBytes;
    const DerDwordReader<CheckedFetch> rd{{data, data_bytes, off[i], limit, &bad}, (uint32_t)(off[i] & 3)};
    parsed[i] = run(rd, len[i], out_rs + 64 * i);
  }
  return bad;
}

}  // extern "C"

#ifdef DER_MAIN
// corpus file: u32 count, then per case u32 claimed length, u32 real bytes,
// the bytes, u8 parsed, 64 B r||s (the expectation, written by the test)
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  uint64_t bad = 0, parsed_total = 0;
  for (uint32_t c = 0; c < count; ++c) {
    uint32_t claim = 0, real = 0;
    uint8_t want_ok = 0, want[64], got[64];
    if (std::fread(&claim, 4, 1, f) != 1 || std::fread(&real, 4, 1, f) != 1) return 2;
    uint8_t* block = static_cast<uint8_t*>(std::malloc(real ? real : 1));  // exactly the encoding's bytes
    if (real && std::fread(block, 1, real, f) != real) return 2;
    if (std::fread(&want_ok, 1, 1, f) != 1 || std::fread(want, 1, 64, f) != 64) return 2;
    const uint8_t ok = run(DerPtrReader{real ? block : nullptr}, claim, got);
    if (ok != want_ok || std::memcmp(got, want, 64) != 0) {
      ++bad;
      std::printf("case %u: parsed %u, want %u\n", c, ok, want_ok);
    }
    parsed_total += ok;
    std::free(block);
  }
  std::fclose(f);
  std::printf("der: %llu mismatches over %u encodings, %llu parsed\n", (unsigned long long)bad, count,
              (unsigned long long)parsed_total);
  return bad ? 1 : 0;
}
#endif
