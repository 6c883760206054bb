// test_tally_mirror.cpp -- TEST PROGRAM: ConsensusTable::FlushPreparesTally /
// FlushCommitsTally (the quorum count taken from Crypto::FlushVotesTally)
// against the existing FlushPrepares / FlushCommits on random multi-sequence
// snapshots: same accepted, applied, errors, commits, replies, stages and
// stored votes, flush after flush (so the second flush of a table runs on the
// signer sets the first one stored).
//
//   ./test_tally_mirror oracle  -- CPU: the oracle behind pbft::Crypto (a test double)
//   ./test_tally_mirror gpu     -- MI355X: GpuCrypto (pbftv_flush_votes, then the
//                                  same host reduce of csrc/tally.h)
#include <array>
#include <cstdio>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../oracle/oracle.h"
#include "pbft.h"

using namespace pbft;

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (c) ++g_pass;                                                          \
    else {                                                                    \
      ++g_fail;                                                               \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                         \
  } while (0)

class OracleCrypto : public Crypto {
 public:
  std::vector<Digest32> Sha256(const std::vector<std::vector<uint8_t>>& msgs) override {
    std::vector<Digest32> out(msgs.size());
    for (size_t i = 0; i < msgs.size(); ++i) oracle_sha256(msgs[i].data(), msgs[i].size(), out[i].data());
    return out;
  }
  std::vector<bool> Verify(const std::vector<Digest32>& h, const std::vector<Sig>& s,
                           const std::vector<uint32_t>& k) override {
    std::vector<bool> out(h.size());
    for (size_t i = 0; i < h.size(); ++i)
      out[i] = k[i] < keys_.size() && oracle_ecdsa_p256_verify(h[i].data(), s[i].data(), keys_[k[i]].data()) == 1;
    return out;
  }
  void RegisterKeys(const std::vector<std::array<uint8_t, 64>>& pub) override { keys_ = pub; }

 private:
  std::vector<std::array<uint8_t, 64>> keys_;
};

struct Signer {
  std::array<uint8_t, 32> d{};
  uint64_t nonce = 1;
  Sig sign(const std::vector<uint8_t>& m) {
    Digest32 h;
    oracle_sha256(m.data(), m.size(), h.data());
    Sig s{};
    for (;;) {
      std::array<uint8_t, 32> k{};
      for (int i = 0; i < 8; ++i) k[31 - i] = (uint8_t)((nonce * 0x9E3779B97F4A7C15ull) >> (8 * i));
      k[0] = d[0] ^ 0x5A;
      ++nonce;
      if (oracle_ecdsa_p256_sign(h.data(), d.data(), k.data(), s.data())) return s;
    }
  }
};

constexpr int64_t kView = 7;
constexpr int kNodes = 37;  // more than one signer word

static bool same_vote(const VoteMsg& a, const VoteMsg& b) {
  return a.ViewID == b.ViewID && a.SequenceID == b.SequenceID && a.Digest == b.Digest && a.NodeID == b.NodeID &&
         a.Type == b.Type && a.Signature == b.Signature;
}

static void same_outcome(const ConsensusTable::FlushOutcome& a, const ConsensusTable::FlushOutcome& b) {
  CHECK(a.accepted == b.accepted);
  CHECK(a.applied == b.applied);
  CHECK(a.errors == b.errors);
  CHECK(a.commits.size() == b.commits.size());
  for (size_t i = 0; i < a.commits.size() && i < b.commits.size(); ++i) CHECK(same_vote(a.commits[i], b.commits[i]));
  CHECK(a.replies.size() == b.replies.size());
  for (size_t i = 0; i < a.replies.size() && i < b.replies.size(); ++i) {
    CHECK(a.replies[i].first.Timestamp == b.replies[i].first.Timestamp);
    CHECK(a.replies[i].first.ClientID == b.replies[i].first.ClientID);
    CHECK(a.replies[i].second.SequenceID == b.replies[i].second.SequenceID);
  }
}

static void same_tables(ConsensusTable& a, ConsensusTable& b, int64_t seq0, int K) {
  CHECK(a.LastCommitted() == b.LastCommitted());
  for (int k = 0; k < K; ++k) {
    State *x = a.Find(seq0 + k), *y = b.Find(seq0 + k);
    CHECK(x && y);
    if (!x || !y) continue;
    CHECK(x->CurrentStage == y->CurrentStage && x->LastSequenceID == y->LastSequenceID);
    for (int which = 0; which < 2; ++which) {
      const auto& m = which ? x->MsgLogs_.CommitMsgs : x->MsgLogs_.PrepareMsgs;
      const auto& w = which ? y->MsgLogs_.CommitMsgs : y->MsgLogs_.PrepareMsgs;
      CHECK(m.size() == w.size());
      for (auto& kv : m) {
        auto it = w.find(kv.first);
        CHECK(it != w.end() && same_vote(kv.second, it->second));
      }
    }
  }
}

static void run(Crypto& c, uint32_t seed) {
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (uint32_t)n); };
  KeyTable keys;
  std::vector<Signer> node(kNodes);
  std::vector<std::string> name(kNodes);
  std::vector<std::array<uint8_t, 64>> pub(kNodes);
  for (int i = 0; i < kNodes; ++i) {
    node[i].d[31] = (uint8_t)(i + 1);
    node[i].d[0] = (uint8_t)(0x21 + i);
    oracle_p256_pubkey(node[i].d.data(), pub[i].data());
    name[i] = "node" + std::to_string(i);
    keys.Add(name[i], (uint32_t)i);
  }
  c.RegisterKeys(pub);
  const int K = 9;
  const int64_t seq0 = 5000 + seed;
  ConsensusTable classic(kView), tally(kView);
  std::vector<std::string> dg(K);
  for (int k = 0; k < K; ++k) {
    RequestMsg r;
    r.Timestamp = 100 + k;
    r.ClientID = "client" + std::to_string(k);
    r.Operation = "op" + std::to_string(k);
    RequestMsg r2 = r;
    auto p1 = classic.Open(seq0 + k).StartConsensus(c, r, seq0 + k);
    auto p2 = tally.Open(seq0 + k).StartConsensus(c, r2, seq0 + k);
    CHECK(p1.value && p2.value && p1.value->Digest == p2.value->Digest);
    dg[k] = p1.value->Digest;
  }
  // a snapshot of votes in random order: per sequence 0..3 voters (so some
  // states need a second flush, some never get there), duplicates (a node
  // voting twice, the copies differently signed or spoilt), a flipped
  // signature, a wrong digest, a wrong view, an unknown node, a stray sequence
  auto snapshot = [&](MsgType type, const std::vector<int>& live) {
    std::vector<VoteMsg> snap;
    for (int k : live) {
      const int voters = pick(4);
      for (int j = 0; j < voters + pick(3); ++j) {
        const int who = j < voters ? pick(kNodes) : pick(3);  // (the extra ones collide often)
        VoteMsg v;
        v.ViewID = kView;
        v.SequenceID = seq0 + k;
        v.Digest = dg[k];
        v.NodeID = name[who];
        v.Type = type;
        const int spoil = pick(10);
        if (spoil == 0) v.Digest[3] = v.Digest[3] == 'a' ? 'b' : 'a';
        if (spoil == 1) v.ViewID = kView + 1;
        if (spoil == 2) v.NodeID = "stranger" + std::to_string(who);
        v.Signature = node[who].sign(Marshal(v));
        if (spoil == 3) v.Signature[9] ^= 0x40;
        if (spoil == 4) v.SequenceID = seq0 - 1 - k;  // no state for it (signed before: the signature fails too)
        snap.push_back(v);
      }
    }
    for (size_t i = snap.size(); i > 1; --i) std::swap(snap[i - 1], snap[(size_t)pick((int)i)]);
    return snap;
  };
  std::vector<int> all(K);
  for (int k = 0; k < K; ++k) all[k] = k;
  size_t prepared = 0, committed = 0, applied = 0, skipped = 0;
  for (int round = 0; round < 3; ++round) {
    const auto snap = snapshot(PrepareMsg, all);
    const auto a = classic.FlushPrepares(c, keys, snap);
    const auto b = tally.FlushPreparesTally(c, keys, snap);
    same_outcome(a, b);
    same_tables(classic, tally, seq0, K);
    prepared += a.commits.size();
    for (size_t i = 0; i < snap.size(); ++i) {
      applied += a.applied[i];
      skipped += a.accepted[i] && !a.applied[i];
    }
  }
  for (int round = 0; round < 3; ++round) {
    const auto snap = snapshot(CommitMsg, all);
    const auto a = classic.FlushCommits(c, keys, snap);
    const auto b = tally.FlushCommitsTally(c, keys, snap);
    same_outcome(a, b);
    same_tables(classic, tally, seq0, K);
    committed += a.replies.size();
  }
  // an empty snapshot changes nothing and returns empty outcomes
  const auto e = tally.FlushPreparesTally(c, keys, {});
  CHECK(e.accepted.empty() && e.commits.empty());
  same_tables(classic, tally, seq0, K);
  std::printf("seed %u: %zu prepared, %zu committed, %zu applied, %zu accepted after the quorum\n", seed, prepared,
              committed, applied, skipped);
  CHECK(prepared > 0 && applied > 0);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "oracle";
  std::unique_ptr<Crypto> c;
  if (mode == "gpu") {
    try {
      c = std::make_unique<GpuCrypto>();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "GpuCrypto: %s\n", e.what());
      return 3;
    }
  } else {
    c = std::make_unique<OracleCrypto>();
  }
  size_t seeds = mode == "gpu" ? 2 : 6;
  for (uint32_t s = 1; s <= seeds; ++s) run(*c, s);
  std::printf("%s: %d checks passed, %d failed\n", mode.c_str(), g_pass, g_fail);
  return g_fail ? 1 : 0;
}
