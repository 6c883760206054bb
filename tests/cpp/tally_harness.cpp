// tally.h on the host for tests/test_tally_cpu.py: the matrix build and the
// per-state reduce exactly as host/pbft.cpp's Crypto::FlushVotesTally runs
// them.  With -DTALLY_MAIN it is a
// stand-alone program (built with -fsanitize=address,undefined) that reads a
// corpus of cases with their expected outputs and runs every state's reduce
// over a row and a signer block allocated at exactly their sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple_pbft_amd/csrc/tally.h"

using namespace pbftv;

extern "C" {

// the whole tally of one case; signers: n_states * W words in/out (null: none);
// quorum_at may be null
void h_tally(const uint8_t* sig, const uint8_t* msg, const uint32_t* key_idx, const uint32_t* state_idx, uint64_t n,
             uint32_t n_states, uint32_t n_signers, uint32_t quorum, uint32_t* signers, uint32_t* count,
             uint32_t* quorum_at) {
  std::vector<uint32_t> first((size_t)n_states * n_signers, kTallyNone);
  tally_first_host(sig, msg, key_idx, state_idx, n, 0, n_states, n_signers, first.data());
  const uint32_t W = tally_words(n_signers);
  for (uint32_t s = 0; s < n_states; ++s)
    tally_reduce_row(first.data() + (size_t)s * n_signers, n_signers, (uint32_t)n, quorum,
                     signers ? signers + (size_t)s * W : nullptr, count + s, quorum_at ? quorum_at + s : nullptr);
}

uint32_t h_tally_words(uint32_t n_signers) { return tally_words(n_signers); }
uint32_t h_tally_word_mask(uint32_t w, uint32_t n_signers) { return tally_word_mask(w, n_signers); }
uint32_t h_tally_index_bits(uint32_t n) { return tally_index_bits(n); }

}  // extern "C"

#ifdef TALLY_MAIN
namespace {

template <class T>
T* exact(const std::vector<uint8_t>& blob, size_t& pos, size_t count) {
  // a heap block of exactly count elements (at least one byte so malloc returns a block)
  T* p = static_cast<T*>(malloc(count * sizeof(T) ? count * sizeof(T) : 1));
  if (pos + count * sizeof(T) > blob.size()) {
    fprintf(stderr, "corpus truncated\n");
    exit(2);
  }
  memcpy(p, blob.data() + pos, count * sizeof(T));
  pos += count * sizeof(T);
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> blob;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + k);
  fclose(f);
  size_t pos = 0;
  uint64_t cases = 0, states = 0, bad = 0;
  while (pos < blob.size()) {
    uint32_t* h = exact<uint32_t>(blob, pos, 6);
    const uint32_t n = h[0], n_states = h[1], n_signers = h[2], quorum = h[3], has_msg = h[4], has_priors = h[5];
    free(h);
    const uint32_t W = tally_words(n_signers);
    uint8_t* sig = exact<uint8_t>(blob, pos, (n + 7) / 8);
    uint8_t* msg = has_msg ? exact<uint8_t>(blob, pos, (n + 7) / 8) : nullptr;
    uint32_t* key = exact<uint32_t>(blob, pos, n);
    uint32_t* st = exact<uint32_t>(blob, pos, n);
    uint32_t* first = static_cast<uint32_t*>(malloc((size_t)n_states * n_signers * 4 ? (size_t)n_states * n_signers * 4 : 1));
    memset(first, 0xFF, (size_t)n_states * n_signers * 4);
    tally_first_host(sig, msg, key, st, n, 0, n_states, n_signers, first);
    for (uint32_t s = 0; s < n_states; ++s) {
      // this state's row and signer words, each in a block of its own size
      uint32_t* row = static_cast<uint32_t*>(malloc(n_signers * 4 ? n_signers * 4 : 1));
      memcpy(row, first + (size_t)s * n_signers, (size_t)n_signers * 4);
      uint32_t* signers = has_priors ? exact<uint32_t>(blob, pos, W) : nullptr;
      uint32_t* want_signers = exact<uint32_t>(blob, pos, W);
      uint32_t* want = exact<uint32_t>(blob, pos, 2);
      uint32_t count = 0xEEEEEEEE, at = 0xEEEEEEEE;
      tally_reduce_row(row, n_signers, n, quorum, signers, &count, &at);
      bool ok = count == want[0] && at == want[1];
      if (signers) ok = ok && memcmp(signers, want_signers, (size_t)W * 4) == 0;
      bad += !ok;
      ++states;
      free(row);
      free(signers);
      free(want_signers);
      free(want);
    }
    free(first);
    free(sig);
    free(msg);
    free(key);
    free(st);
    ++cases;
  }
  printf("tally: %llu mismatches over %llu states of %llu cases\n", (unsigned long long)bad,
         (unsigned long long)states, (unsigned long long)cases);
  return bad ? 1 : 0;
}
#endif
