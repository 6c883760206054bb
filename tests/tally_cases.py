"""Case generators for the quorum tally (tests/tally_model.py states what is
computed).  One suite per signer-universe size; every suite is checked here,
with the model alone, to hold at least one state each whose quorum_at is NONE,
BEFORE and a real index.

Sizes: n_signers around the word (32) and the 64-signer seams and far beyond
(1000, 2049: many words per state); n around 64 and 256 and beyond.  Per-vote shapes: duplicate (state, signer) votes
with an earlier rejected copy and a later accepted one, votes with one of the
two bits only, state_idx == n_states and 0xFFFFFFFF, key_idx >= n_signers with
its signature bit set, first-indices descending in key order.  Priors:
overlapping the new signers, garbage bits at or above n_signers, already at the
quorum; quorum in {0, 1, 2, n_signers, n_signers + 1}; the quorum completed at
index 0 and at index n - 1; states with no votes."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import tally_model as tm

N_SIGNERS = [1, 31, 32, 33, 63, 64, 65, 100, 1000, 2049]
N_VOTES = [0, 1, 63, 64, 65, 257, 1000]


@dataclass
class Case:
    name: str
    n_states: int
    n_signers: int
    quorum: int
    sig: np.ndarray        # (n,) bool
    msg: np.ndarray        # (n,) bool
    key_idx: np.ndarray    # (n,) uint32
    state_idx: np.ndarray  # (n,) uint32
    priors: np.ndarray     # (n_states, W) uint32

    @property
    def n(self):
        return len(self.sig)

    def sig_bitmap(self):
        return np.packbits(self.sig, bitorder="little") if self.n else np.zeros(0, np.uint8)

    def msg_bitmap(self):
        return np.packbits(self.msg, bitorder="little") if self.n else np.zeros(0, np.uint8)

    def expect(self, with_msg=True, with_priors=True):
        return _expect(self, with_msg, with_priors)


_cache: dict = {}


def _expect(c, with_msg, with_priors):
    key = (id(c), with_msg, with_priors)
    if key not in _cache:
        _cache[key] = tm.tally(c.sig, c.msg if with_msg else None, c.key_idx, c.state_idx, c.n_states, c.n_signers,
                               c.quorum, c.priors if with_priors else None)
    return _cache[key]


def quorums(n_signers):
    return [0, 1, 2, n_signers, n_signers + 1]


def _priors(rng, n_states, n_signers, quorum):
    """state 0: none; 1: a random subset (overlaps the voters); 2: the same with
    garbage at and above n_signers; 3: at the quorum already; others random"""
    W = tm.words(n_signers)
    P = np.zeros((n_states, W), np.uint32)
    for s in range(1, n_states):
        kind = s if s < 4 else int(rng.integers(0, 4))
        if kind == 3:
            chosen = rng.permutation(n_signers)[:min(quorum, n_signers)]
        else:
            chosen = np.nonzero(rng.random(n_signers) < 0.3)[0]
        P[s] = tm.to_words([int(k) for k in chosen], n_signers)
        if kind == 2 and n_signers % 32:
            P[s, W - 1] |= np.uint32((0xFFFFFFFF << (n_signers % 32)) & 0xFFFFFFFF)
    return P


def random_case(n_signers, n, quorum, seed):
    rng = np.random.default_rng(seed)
    n_states = 6 if n < 257 else 10  # the last state never gets a vote
    live = n_states - 1
    state_idx = rng.integers(0, live, n).astype(np.uint32)
    # few signers per state relative to the votes when n is large: duplicates
    key_idx = rng.integers(0, n_signers, n).astype(np.uint32)
    sig = rng.random(n) < 0.75
    msg = rng.random(n) < 0.75
    for i in range(0, n, 7):  # out-of-range states and keys, their bits set
        kind = (i // 7) % 5
        sig[i] = msg[i] = True
        if kind == 0:
            state_idx[i] = n_states
        elif kind == 1:
            state_idx[i] = 0xFFFFFFFF
        elif kind == 2:
            key_idx[i] = n_signers
        elif kind == 3:
            key_idx[i] = 0xFFFFFFFF
        else:
            key_idx[i] = n_signers + 31
    for i in range(3, n - 5, 11):  # an earlier rejected copy, a later accepted one, a third after it
        j, k = i + 2, i + 4
        state_idx[j] = state_idx[k] = state_idx[i] = state_idx[i] % live
        key_idx[j] = key_idx[k] = key_idx[i] = key_idx[i] % n_signers
        sig[i], msg[i] = (i // 11) % 2 == 0, (i // 11) % 2 == 1  # one bit only
        sig[j] = msg[j] = True
        sig[k] = msg[k] = True
    return Case("random n_signers=%d n=%d quorum=%d" % (n_signers, n, quorum), n_states, n_signers, quorum, sig, msg,
                key_idx, state_idx, _priors(rng, n_states, n_signers, quorum))


def descending_case(n_signers, quorum):
    """state 0: vote i comes from signer n_signers - 1 - i, so the r-th smallest
    first-index belongs to the r-th LARGEST key; state 1 the same under priors"""
    m = min(n_signers, 300)
    n = 2 * m
    key_idx = np.concatenate([np.arange(n_signers - 1, n_signers - 1 - m, -1)] * 2).astype(np.uint32)
    state_idx = np.repeat(np.array([0, 1], np.uint32), m)
    P = np.zeros((3, tm.words(n_signers)), np.uint32)
    P[1] = tm.to_words(range(n_signers - 1, -1, -3), n_signers)
    return Case("descending n_signers=%d quorum=%d" % (n_signers, quorum), 3, n_signers, quorum, np.ones(n, bool),
                np.ones(n, bool), key_idx, state_idx, P)


def edge_case(n_signers, n):
    """the quorum completed by vote 0 and by vote n - 1.  State 0: vote 0 alone,
    from the last signer, under priors one short of the quorum.  State 1: the
    votes 1 .. n - 2 cycle over d - 1 signers and vote n - 1 brings the d-th,
    with quorum = d."""
    assert n >= 2
    d = min(n - 1, n_signers)
    key_idx = np.zeros(n, np.uint32)
    state_idx = np.ones(n, np.uint32)
    sig = np.ones(n, bool)
    state_idx[0] = 0
    key_idx[0] = n_signers - 1
    if d > 1:
        key_idx[1:n - 1] = np.arange(n - 2) % (d - 1)
    else:
        sig[1:n - 1] = False  # one signer: only the last vote counts
    key_idx[n - 1] = d - 1
    P = np.zeros((2, tm.words(n_signers)), np.uint32)
    P[0] = tm.to_words(range(0, d - 1), n_signers)  # (d - 1 <= n_signers - 1: the last signer is new)
    c = Case("edge n_signers=%d n=%d" % (n_signers, n), 2, n_signers, d, sig, np.ones(n, bool), key_idx, state_idx, P)
    _, _, q = c.expect()
    assert int(q[0]) == 0 and int(q[1]) == n - 1, (c.name, q)
    return c


@functools.lru_cache(maxsize=None)
def suite(n_signers):
    """every case of one signer-universe size"""
    out = []
    for qi, quorum in enumerate(quorums(n_signers)):
        for n in N_VOTES:
            out.append(random_case(n_signers, n, quorum, 1000 * n_signers + 10 * n + qi))
        out.append(descending_case(n_signers, quorum))
    for n in (2, 64, 65, 257):
        out.append(edge_case(n_signers, n))
    kinds = set()
    at0 = at_last = False
    for c in out:
        _, _, q = c.expect()
        for s in range(c.n_states):
            v = int(q[s])
            kinds.add("none" if v == tm.NONE else "before" if v == tm.BEFORE else "index")
            at0 |= v == 0
            at_last |= c.n > 1 and v == c.n - 1
    assert kinds == {"none", "before", "index"}, (n_signers, kinds)
    assert at0 and at_last, (n_signers, at0, at_last)
    return out


def all_cases():
    return [c for k in N_SIGNERS for c in suite(k)]
