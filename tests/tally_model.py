"""The quorum tally of a vote snapshot, stated in plain Python (include/pbftv.h,
"quorum tally"; simple_pbft_amd/csrc/tally.h): the model every form of the
tally -- tally.h on the host, the kernels, the tallying flushes -- is compared
with, word for word."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
BEFORE = 0xFFFFFFFE


def words(n_signers: int) -> int:
    return (n_signers + 31) // 32


def to_words(signer_set, n_signers: int) -> list[int]:
    w = [0] * words(n_signers)
    for k in signer_set:
        w[k // 32] |= 1 << (k % 32)
    return w


def from_words(ws, n_signers: int) -> set[int]:
    """the signers of one state's words; bits at positions >= n_signers are ignored"""
    return {k for k in range(n_signers) if (int(ws[k // 32]) >> (k % 32)) & 1}


def tally(sig, msg, key_idx, state_idx, n_states, n_signers, quorum, priors=None):
    """sig / msg: per-vote booleans (msg None: all set); priors: (n_states, W)
    words or None.  Returns (signers (n_states, W) uint32, count (n_states,)
    uint32, quorum_at (n_states,) uint32)."""
    n = len(sig)
    first = [dict() for _ in range(n_states)]
    for i in range(n):
        s, k = int(state_idx[i]), int(key_idx[i])
        if sig[i] and (msg is None or msg[i]) and s < n_states and k < n_signers:
            first[s].setdefault(k, i)  # votes come in index order: the first one stays
    W = words(n_signers)
    signers = np.zeros((n_states, W), np.uint32)
    count = np.zeros(n_states, np.uint32)
    q_at = np.zeros(n_states, np.uint32)
    for s in range(n_states):
        P = from_words(priors[s], n_signers) if priors is not None else set()
        union = P | set(first[s])
        signers[s] = to_words(union, n_signers)
        count[s] = len(union)
        if len(P) >= quorum:
            q_at[s] = BEFORE
            continue
        r = quorum - len(P)
        F = sorted(i for k, i in first[s].items() if k not in P)
        q_at[s] = NONE if len(F) < r else F[r - 1]
    return signers, count, q_at


def applied(sig, msg, key_idx, state_idx, n_states, n_signers, q_at):
    """the mirror's applied[i]: a counting vote is applied iff its state's
    quorum_at is NONE or i <= quorum_at"""
    out = []
    for i in range(len(sig)):
        s, k = int(state_idx[i]), int(key_idx[i])
        counts = bool(sig[i]) and (msg is None or bool(msg[i])) and s < n_states and k < n_signers
        out.append(counts and (int(q_at[s]) == NONE or i <= int(q_at[s])))
    return out
