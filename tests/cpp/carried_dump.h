// carried_dump.h -- TEST INFRASTRUCTURE ONLY.
//
// Reader of the compact dump tests/test_carried_cases.py writes of
// carried_cases.combined() for the stand-alone (sanitizer) builds of
// varbase_harness.cpp and sec1_harness.cpp.  Layout, little-endian:
//   "CARRIED1", uint64 n, then column after column:
//   hashes 32 n | r||s 64 n | keys X||Y 64 n | keys compressed 33 n |
//   expected bit under X||Y n | expected bit under the compressed key n |
//   rerun n (0 / 1: pinned off / on, 255: not pinned) |
//   Python's decode of the compressed key: accepted n, X||Y 64 n (zeros if not)
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct CarriedDump {
  uint64_t n = 0;
  std::vector<uint8_t> hashes, sigs, xy, comp, want_xy, want_comp, rerun, comp_ok, comp_xy;

  bool read(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char magic[8];
    bool ok = fread(magic, 1, 8, f) == 8 && !memcmp(magic, "CARRIED1", 8) && fread(&n, 8, 1, f) == 1 && n < (1u << 24);
    auto col = [&](std::vector<uint8_t>& v, uint64_t each) {
      v.resize(n * each);
      ok = ok && fread(v.data(), 1, v.size(), f) == v.size();
    };
    if (ok) {
      col(hashes, 32);
      col(sigs, 64);
      col(xy, 64);
      col(comp, 33);
      col(want_xy, 1);
      col(want_comp, 1);
      col(rerun, 1);
      col(comp_ok, 1);
      col(comp_xy, 64);
      ok = ok && fgetc(f) == EOF;
    }
    fclose(f);
    return ok;
  }
};
