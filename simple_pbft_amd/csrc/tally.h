// tally.h -- quorum tally of a vote snapshot: per consensus state, which
// signers have a counting vote, how many, and which vote completed the quorum.
// What the caller of a vote flush does with its two bitmaps (drop duplicate
// signers per state, count up to 2f, note where the state advanced), stated
// once: host/pbft.cpp's Crypto::FlushVotesTally and the CPU harness
// tests/cpp/tally_harness.cpp run it.  The selection (tally_quorum_at) is
// written for the host and the device alike (the count is a functor: a loop
// over the row here, a wave ballot in a kernel); no kernel uses it yet.
//
// A vote i counts iff its signature bit and its message bit are set,
// state_idx[i] < n_states and key_idx[i] < n_signers.  first[s * n_signers + k]
// is the smallest counting i of state s and signer k, kTallyNone where there is
// none (tally_first_host).  Per state s, with P the prior signer set
// (W = tally_words(n_signers) little-endian words, bit k in word k / 32 at bit
// k % 32, bits at positions >= n_signers ignored and written back 0):
//   signers  = P | {k : first[s][k] != kTallyNone}           (bits >= n_signers 0)
//   count    = popcount(signers)
//   quorum_at= kTallyBefore             if |P| >= quorum     (covers quorum == 0)
//              kTallyNone               if |F| < r,  r = quorum - |P|,
//                                       F = {first[s][k] : k not in P, != kTallyNone}
//              the r-th smallest of F   otherwise: the snapshot index of the
//                                       vote that completes the quorum when the
//                                       votes are applied in order
// The elements of F are distinct vote indices below n < kTallyBefore.  A
// counting vote is applied by its state iff quorum_at is kTallyNone or
// i <= quorum_at (the MSGENOUGH break of node.go:564-566).
//
// The selection is a bitwise binary search on the index value: the answer is
// the largest x with |{f in F : f < x}| < r, built from the top bit of n - 1
// down, one count per bit (at most 32).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBFTV_TALLY_HD __host__ __device__ __forceinline__
#else
#define PBFTV_TALLY_HD inline
#endif

namespace pbftv {

constexpr uint32_t kTallyNone = 0xFFFFFFFFu;    // quorum_at: the state has not reached its quorum
constexpr uint32_t kTallyBefore = 0xFFFFFFFEu;  // quorum_at: the prior signers alone had reached it
constexpr uint64_t kTallyMaxCells = 1ull << 28;  // n_states * n_signers: one uint32 each, 1 GiB

PBFTV_TALLY_HD uint32_t tally_words(uint32_t n_signers) { return n_signers / 32u + (n_signers % 32u != 0u); }

// the bits of signer word w that name a signer below n_signers
PBFTV_TALLY_HD uint32_t tally_word_mask(uint32_t w, uint32_t n_signers) {
  const uint64_t lo = 32ull * w;
  if (lo + 32u <= n_signers) return 0xFFFFFFFFu;
  if (lo >= n_signers) return 0u;
  return (1u << (n_signers - (uint32_t)lo)) - 1u;
}

PBFTV_TALLY_HD uint32_t tally_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// rounds of the search: the bits of the largest index, n - 1 (0 for n <= 1)
PBFTV_TALLY_HD uint32_t tally_index_bits(uint32_t n) {
  uint32_t b = 0;
  while (b < 32u && ((uint64_t)1 << b) < n) ++b;
  return b;
}

// quorum_at of one state.  prior_count = |P|, fresh = |F|, n = the snapshot's
// vote count (every element of F is below it), count_lt(x) = |{f in F : f < x}|
// for 0 < x < 2^32.
template <class CountLt>
PBFTV_TALLY_HD uint32_t tally_quorum_at(uint32_t prior_count, uint32_t quorum, uint32_t fresh, uint32_t n,
                                        CountLt count_lt) {
  if (prior_count >= quorum) return kTallyBefore;
  const uint32_t r = quorum - prior_count;
  if (fresh < r) return kTallyNone;
  uint32_t x = 0;
  for (uint32_t b = tally_index_bits(n); b-- > 0u;) {
    const uint32_t t = x | (1u << b);
    if (count_lt(t) < r) x = t;
  }
  return x;
}

// ---- host side ----

// One state on the host: row = its n_signers first-indices; signers = its W
// prior words in, the union out (null: no priors, nothing written); *count and
// *quorum_at (may be null) as defined above.
inline void tally_reduce_row(const uint32_t* row, uint32_t n_signers, uint32_t n, uint32_t quorum, uint32_t* signers,
                             uint32_t* count, uint32_t* quorum_at) {
  const uint32_t W = tally_words(n_signers);
  auto prior_word = [&](uint32_t w) { return signers ? signers[w] & tally_word_mask(w, n_signers) : 0u; };
  auto voted_word = [&](uint32_t w) {
    uint32_t voted = 0;
    const uint32_t hi = n_signers - 32u * w < 32u ? n_signers - 32u * w : 32u;
    for (uint32_t b = 0; b < hi; ++b) voted |= (uint32_t)(row[32u * w + b] != kTallyNone) << b;
    return voted;
  };
  uint32_t prior_count = 0, all = 0, fresh = 0;
  for (uint32_t w = 0; w < W; ++w) {
    const uint32_t prior = prior_word(w), voted = voted_word(w);
    prior_count += tally_popc(prior);
    all += tally_popc(prior | voted);
    fresh += tally_popc(voted & ~prior);
  }
  *count = all;
  if (quorum_at)  // (before the union replaces the priors: F leaves the prior signers out)
    *quorum_at = tally_quorum_at(prior_count, quorum, fresh, n, [&](uint32_t x) {
      uint32_t c = 0;
      for (uint32_t w = 0; w < W; ++w) {
        const uint32_t open = ~prior_word(w) & tally_word_mask(w, n_signers);
        for (uint32_t b = 0; b < 32u && (open >> b) != 0u; ++b) c += ((open >> b) & 1u) && row[32u * w + b] < x;
      }
      return c;
    });
  if (signers)
    for (uint32_t w = 0; w < W; ++w) signers[w] = prior_word(w) | voted_word(w);
}

// The matrix on the host: first must
// hold n_states * n_signers words of kTallyNone on entry; vote i is recorded
// under the index base + i.  sig / msg: LSB-first bitmaps (msg null: all ones).
inline void tally_first_host(const uint8_t* sig, const uint8_t* msg, const uint32_t* key_idx,
                             const uint32_t* state_idx, uint64_t n, uint32_t base, uint32_t n_states,
                             uint32_t n_signers, uint32_t* first) {
  for (uint64_t i = 0; i < n; ++i) {
    if (!((sig[i >> 3] >> (i & 7)) & 1u) || (msg && !((msg[i >> 3] >> (i & 7)) & 1u))) continue;
    const uint32_t s = state_idx[i], k = key_idx[i];
    if (s >= n_states || k >= n_signers) continue;
    uint32_t& f = first[(uint64_t)s * n_signers + k];
    const uint32_t v = base + (uint32_t)i;
    if (v < f) f = v;
  }
}

}  // namespace pbftv
