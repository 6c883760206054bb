"""Case lists for the signer's stage kernels (simple_pbft_amd/csrc/p256_sign.hip:
k_sign_nonce, k_sign_comb, k_sign_tail), run one at a time on records the test
writes (tests/cpp/sign_stage_probe.hip, tests/test_gpu_sign_stages.py).  Built
on tests/sign_cases.py; every expected value comes from tests/rfc6979_model.py,
oracle/p256.py and plain Python integers, never from the code under test.  The
model is pure Python, so signatures are computed once per distinct (hash, key)
and the lists of sign_cases are reused through their caches.

The record between the stages (SignRec, 128 bytes) as 32 little-endian words:
  0..7 k   8..15 k^-1   16 state   17 candidate index   18..19 zero
  20..27 r   28..31 unused
The nonce stage owns words 0..19, the comb words 16 and 20..27, the tail words
0..15 (it writes zeros there: k and k^-1 do not outlive the batch).

A record in state "walk met" is NEVER combined with a key index that is out of
range or names an invalid key: the comb raises that state only on a record the
nonce stage made, and the nonce stage makes none without a valid key, so the
tail loads the key of such a row without asking again.  A forged pairing would
make it read outside the key array.  check_met_rows() asserts this over every
list here and the probe refuses such an input."""
from __future__ import annotations

import functools

import numpy as np

import rfc6979_model as model
import sign_cases as sc

N, TOP = sc.N, sc.TOP
REC_WORDS = 32
K, KINV, STATE, CAND, R = 0, 8, 16, 17, 20  # word offsets
NONE, NONCE_READY, R_READY, WALK_MET = 0, 1, 2, 3
BIG = 0xFFFFFFFF
JUNK = 0x5A5A0000  # + the word's index: what a stage does not own must come back unchanged


def words(v: int) -> np.ndarray:
    """a 256-bit integer as 8 little-endian words"""
    return np.frombuffer(v.to_bytes(32, "little"), np.uint32).copy()


def blank_records(n: int) -> np.ndarray:
    """n + 1 records of junk, a different word at every index; the last one is the guard"""
    return np.tile(JUNK + np.arange(REC_WORDS, dtype=np.uint32), (n + 1, 1))


def put(rec_row, state, k=None, kinv=None, r=None, cand=0):
    for at, v in ((K, k), (KINV, kinv), (R, r)):
        if v is not None:
            rec_row[at:at + 8] = words(v)
    rec_row[STATE], rec_row[CAND] = state, cand
    rec_row[CAND + 1:CAND + 3] = 0


def key_block(ds) -> np.ndarray:
    """8 words per key, then one validity word per key: what pbftv_register_signing_keys
    uploads (an invalid key's words are zeros)"""
    out = np.zeros(9 * len(ds), np.uint32)
    for j, d in enumerate(ds):
        if 0 < d < N:
            out[8 * j:8 * j + 8] = words(d)
            out[8 * len(ds) + j] = 1
    return out


@functools.lru_cache(maxsize=None)
def signature(h: bytes, d: int) -> bytes:
    return model.sign_bytes(h, d)


@functools.lru_cache(maxsize=None)
def genuine(h: bytes, d: int):
    """(k, k^-1, r) of the model's signature of (h, d): its first candidate is the nonce"""
    k, j = model.nonce(d, h)
    sig = signature(h, d)
    assert j == 0 and any(sig)
    return k, pow(k, -1, N), int.from_bytes(sig[:32], "big")


def check_met_rows(rec, kidx, ds):
    """no "walk met" record beside an out-of-range or invalid key (the module's header)"""
    for i in range(len(kidx)):
        if rec[i, STATE] == WALK_MET:
            assert kidx[i] < len(ds) and 0 < ds[kidx[i]] < N, i


# ---- nonce rows: the bits2octets seam x the ends of the key range, then random pairs ----
@functools.lru_cache(maxsize=None)
def nonce_rows():
    """(hashes, kidx, ds, records in, words 0..19 expected).  Every d is its own key."""
    cases = sc.drbg_cases()
    n = len(cases)
    ds = tuple(d for d, _ in cases)
    rec = blank_records(n)
    want = np.zeros((n, 20), np.uint32)
    for i, (d, h) in enumerate(cases):
        k, j = model.nonce(d, sc.be(h))
        assert j == 0  # the first candidate (a rejected one has probability 2^-32)
        put(want[i], NONCE_READY, k=k, kinv=pow(k, -1, N), cand=0)
    return sc.col([h for _, h in cases]), np.arange(n, dtype=np.uint32), ds, rec, want


@functools.lru_cache(maxsize=None)
def chain_expected():
    """the model's whole signature of every nonce row"""
    cases = sc.drbg_cases()
    return np.frombuffer(b"".join(signature(sc.be(h), d) for d, h in cases), np.uint8).reshape(-1, 64).copy()


# ---- comb rows: every chosen nonce in a record's k words ----
@functools.lru_cache(maxsize=None)
def comb_rows():
    """(records in, records expected).  r = x(kG) mod n is the r of sign_cases.with_k_expected(),
    which takes it from oracle.p256.scalar_mult once per nonce."""
    ks = sc.chosen_k()
    rs, ok = sc.with_k_expected()
    per = len(sc.E_ENDS) * len(sc.D_PAIR)
    assert len(rs) == per * len(ks) and ok.all()
    rec = blank_records(len(ks))
    for i, k in enumerate(ks):
        assert sc.with_k_cases()[per * i][2] == k
        put(rec[i], NONCE_READY, k=k, kinv=pow(k, -1, N))
    want = rec.copy()
    for i in range(len(ks)):
        want[i, R:R + 8] = words(int.from_bytes(rs[per * i, :32].tobytes(), "big"))
        want[i, STATE] = R_READY
    return rec, want


# ---- tail rows with a chosen record ----
def _seeded(seed):
    return int.from_bytes(np.random.default_rng(seed).bytes(32), "big") % (N - 1) + 1


TAIL_R = (1, N - 1, 1 << 32, 1 << 224, _seeded(2024))
TAIL_KINV = (1, 2, N - 1, _seeded(2025))


@functools.lru_cache(maxsize=None)
def tail_cross():
    """every (e, d, r, kinv) of the cross, s = 0 included"""
    return tuple((e, d, r, ki) for r in TAIL_R for ki in TAIL_KINV for e in sc.E_ENDS for d in sc.D_PAIR)


@functools.lru_cache(maxsize=None)
def tail_chosen():
    """(e, d, r, kinv, s) with s = kinv (e + r d) mod n != 0.  A combination whose s is 0
    is dropped (it would be a rerun; those have rows of their own below)."""
    out = []
    for e, d, r, ki in tail_cross():
        s = ki * (e + r * d) % N
        if s:
            out.append((e, d, r, ki, s))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tail_chosen_rows():
    """(hashes, kidx, ds, records in, r||s rows expected) in state "r ready"; k is junk"""
    cases = tail_chosen()
    n = len(cases)
    rec = blank_records(n)
    want = np.zeros((n, 64), np.uint8)
    for i, (e, d, r, ki, s) in enumerate(cases):
        put(rec[i], R_READY, kinv=ki, r=r)
        want[i] = np.frombuffer(sc.be(r) + sc.be(s), np.uint8)
    kidx = np.array([sc.D_PAIR.index(c[1]) for c in cases], np.uint32)
    return sc.col([c[0] for c in cases]), kidx, sc.D_PAIR, rec, want


# ---- the 257-row batch: reruns and rows with no signature among ordinary rows ----
BATCH = 257
ORDINARY = 64                                    # distinct (hash, key) pairs behind the ordinary rows
RERUN_LANES = (0, 1, 31, 32, 62, 63) + tuple(range(64, 128)) + (255, 256)
FULL_WAVE, SINGLE_WAVE = range(64, 128), range(192, 256)  # every lane reruns; lane 255 alone reruns
FORGERIES = ("met", "r0", "kinv0")
RERUN_HASHES = (0, N, TOP)                       # E_ENDS-style hashes beside the random ones
NOSIG_LANES = (7, 8, 9, 10, 130, 189, 200, 254)


@functools.lru_cache(maxsize=None)
def rerun_pairs():
    """24 genuine (hash, valid key) pairs: 21 of random_pairs() and the three end hashes
    under keys of their own"""
    rp = sc.random_pairs()
    return tuple(rp[:21]) + tuple((sc.be(h), rp[ORDINARY + j][1]) for j, h in enumerate(RERUN_HASHES))


@functools.lru_cache(maxsize=None)
def tail_batch():
    """dict of the batch: hashes, kidx, ds (the last key is invalid), rec (in), want (r||s),
    ok, rerun {lane: (pair index, forgery)}, nosig {lane: how}.

    Ordinary rows carry the genuine "r ready" record of their pair.  A rerun row keeps its
    genuine hash and key and a forged record: "met" (state "walk met", junk in r, k and k^-1),
    "r0" (state "r ready", r = 0), "kinv0" (state "r ready", k^-1 = 0, so s = 0); the tail must
    answer with the model's signature all the same.  The 24 pairs x 3 forgeries fill the 72
    rerun lanes."""
    rp = sc.random_pairs()
    pairs = rerun_pairs()
    ds = [d for _, d in rp[:ORDINARY]] + [d for _, d in pairs[21:]] + [0]
    nvalid = len(ds) - 1
    key_of = {d: j for j, d in enumerate(ds)}
    hashes = np.zeros((BATCH, 32), np.uint8)
    kidx = np.zeros(BATCH, np.uint32)
    rec = blank_records(BATCH)
    want = np.zeros((BATCH, 64), np.uint8)
    ok = np.ones(BATCH, bool)
    for i in range(BATCH):  # ordinary everywhere first
        h, d = rp[i % ORDINARY]
        k, ki, r = genuine(h, d)
        hashes[i], kidx[i] = np.frombuffer(h, np.uint8), key_of[d]
        put(rec[i], R_READY, k=k, kinv=ki, r=r)
        want[i] = np.frombuffer(signature(h, d), np.uint8)
    rerun = {}
    assert len(RERUN_LANES) == len(pairs) * len(FORGERIES)
    junk = np.random.default_rng(77)
    for c, lane in enumerate(RERUN_LANES):
        p, how = c % len(pairs), FORGERIES[(c + c // len(pairs)) % 3]
        h, d = pairs[p]
        k, ki, r = genuine(h, d)
        hashes[lane], kidx[lane] = np.frombuffer(h, np.uint8), key_of[d]
        want[lane] = np.frombuffer(signature(h, d), np.uint8)
        rec[lane] = blank_records(0)[0]
        if how == "met":
            rec[lane, :REC_WORDS] = junk.integers(0, 1 << 32, REC_WORDS, dtype=np.uint64).astype(np.uint32)
            put(rec[lane], WALK_MET)
        elif how == "r0":
            put(rec[lane], R_READY, k=k, kinv=ki, r=0)
        else:
            put(rec[lane], R_READY, k=k, kinv=0, r=r)
        rerun[lane] = (p, how)
    hows = [("none", NONE, None), ("none+past", NONE, nvalid + 1), ("past", R_READY, nvalid + 1),
            ("big", R_READY, BIG), ("invalid", R_READY, nvalid), ("none+invalid", NONE, nvalid),
            ("none+big", NONE, BIG), ("past", R_READY, nvalid + 1)]
    nosig = {}
    for lane, (name, state, idx) in zip(NOSIG_LANES, hows):
        rec[lane, STATE] = state  # the rest of the record stays its pair's genuine one
        if idx is not None:
            kidx[lane] = idx
        want[lane], ok[lane] = 0, False
        nosig[lane] = name
    check_met_rows(rec, kidx, ds)
    return dict(hashes=hashes, kidx=kidx, ds=tuple(ds), rec=rec, want=want, ok=ok, rerun=rerun, nosig=nosig)


def bitmap(ok) -> np.ndarray:
    """ok flags -> the LSB-first bitmap, padding bits zero"""
    return np.packbits(np.asarray(ok, bool), bitorder="little")
