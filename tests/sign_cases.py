"""Case lists for the signer (simple_pbft_amd/csrc/sign.h), shared by the CPU
harness test (tests/test_sign_cpu.py), the device probe
(tests/test_gpu_sign_probe.py) and the library tests (tests/test_gpu_sign.py).
Expected values come from tests/rfc6979_model.py alone."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import rfc6979_model as model
from oracle import der as oder
from oracle import p256

N, P = p256.N, p256.P
TOP = (1 << 256) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def be(v: int) -> bytes:
    return v.to_bytes(32, "big")


def col(values) -> np.ndarray:
    """ints -> an (n, 32) big-endian byte column"""
    return np.frombuffer(b"".join(be(v) for v in values), np.uint8).reshape(-1, 32).copy()


# ---- the DRBG: the bits2octets seam crossed with the ends of the key range ----
H1_SEAM = (0, 1, N - 1, N, N + 1, TOP)
D_ENDS = (1, 2, N - 2, N - 1)


@functools.lru_cache(maxsize=None)
def drbg_cases():
    """(d, h1 as int) pairs: the seam cross, then 64 seeded random pairs."""
    out = [(d, h) for h in H1_SEAM for d in D_ENDS]
    rng = np.random.default_rng(6979)
    for _ in range(64):
        d = int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1
        out.append((d, int.from_bytes(rng.bytes(32), "big")))
    return tuple(out)


def drbg_expected(cases, ncand=3) -> np.ndarray:
    out = np.zeros((len(cases), ncand, 32), np.uint8)
    for i, (d, h) in enumerate(cases):
        g = model.candidates(d, be(h))
        for j in range(ncand):
            out[i, j] = np.frombuffer(be(next(g)), np.uint8)
    return out


# ---- chosen nonces: the comb walk's digit seams ----
def _windows(ws) -> int:
    return sum(w << (16 * i) for i, w in enumerate(ws))


@functools.lru_cache(maxsize=None)
def chosen_k():
    """Nonces in (0, n): the ends of the range; every 16-bit window zero but
    one; windows of 0x8000 / 0x8001 / 0x7FFF -- where the signed recoding does
    or does not carry (a window above 0x8000 borrows from the next) -- alone
    in each window and in runs from each window up to the top one; all ones."""
    ks = [1, 2, 3, N - 1, N - 2]
    for i in range(16):
        for v in (1, 0x1234, 0xFFFF):
            ks.append(v << (16 * i))
    for v in (0x8000, 0x8001, 0x7FFF):
        for i in range(16):
            ks.append(v << (16 * i))
            ks.append(_windows([0] * i + [v] * (16 - i)))
    ks += [(1 << 255) - 1, (1 << 224) - 1, int("ffff0000" * 8, 16) >> 1]
    seen, out = set(), []
    for k in ks:
        assert 0 < k < N
        if k not in seen:
            seen.add(k)
            out.append(k)
    return tuple(out)


E_ENDS = (0, N - 1, N, TOP)
D_PAIR = (1, N - 1)


@functools.lru_cache(maxsize=None)
def with_k_cases():
    """(e, d, k) triples: every chosen nonce under every (e, d) of the cross."""
    return tuple((e, d, k) for k in chosen_k() for e in E_ENDS for d in D_PAIR)


@functools.lru_cache(maxsize=None)
def with_k_expected():
    """r||s rows (n, 64) and ok flags of with_k_cases() by the model.  k*G is
    computed once per nonce and handed to the textbook formula's own steps
    through p256.sign on the first (e, d) of each nonce, which pins the cache."""
    cases = with_k_cases()
    rs = np.zeros((len(cases), 64), np.uint8)
    ok = np.zeros(len(cases), bool)
    rx = {}
    for i, (e, d, k) in enumerate(cases):
        if k not in rx:
            got = model.sign_with_k(be(e), d, k)
            rx[k] = p256.scalar_mult(k, p256.G)[0] % N
            assert got is None or got[0] == rx[k]
        else:
            r = rx[k]
            s = pow(k, -1, N) * (e + r * d) % N
            got = None if r == 0 or s == 0 else (r, s)
        if got is not None:
            rs[i] = np.frombuffer(be(got[0]) + be(got[1]), np.uint8)
            ok[i] = True
    return rs, ok


# ---- x mod n as a function of its own ----
# No nonce with R.x >= n can be found (that needs an x in [n, p), 2^-128 of
# all x), so a whole signature never exercises the subtraction: these do.
X_MOD_N = (0, N - 1, N, N + 1, P - 1)

# ---- keys ----
BAD_KEYS = (0, N, TOP)


# ---- whole signatures ----
@functools.lru_cache(maxsize=None)
def keypool(nkeys=5, seed=256):
    rng = np.random.default_rng(seed)
    return tuple(int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(nkeys))


def pubkeys(ds) -> np.ndarray:
    out = np.zeros((len(ds), 64), np.uint8)
    for j, d in enumerate(ds):
        x, y = p256.pubkey(d)
        out[j] = np.frombuffer(be(x) + be(y), np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def random_pairs(n=256, seed=1979):
    """n seeded (h, d) pairs, every d its own key"""
    rng = np.random.default_rng(seed)
    return tuple((rng.bytes(32), int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1) for _ in range(n))


def sign_expected(pairs) -> np.ndarray:
    return np.frombuffer(b"".join(model.sign_bytes(h, d) for h, d in pairs), np.uint8).reshape(-1, 64).copy()


@functools.lru_cache(maxsize=None)
def _batch_rows(nkeys, seed):
    """96 distinct (hash, key index) rows and the model's signatures under keypool(nkeys)"""
    rng = np.random.default_rng(seed)
    hs = [rng.bytes(32) for _ in range(96)]
    ki = rng.integers(0, nkeys, 96)
    ds = keypool(nkeys)
    sig = [model.sign_bytes(hs[i], ds[ki[i]]) for i in range(96)]
    return (np.frombuffer(b"".join(hs), np.uint8).reshape(-1, 32), ki.astype(np.uint32),
            np.frombuffer(b"".join(sig), np.uint8).reshape(-1, 64))


def batch(n, nkeys=5, seed=4096):
    """hashes (n, 32), key indices in mixed order, and the model's signatures
    (n, 64) under keypool(nkeys).  The model runs once per distinct (hash,
    key): a batch of n tiles 96 distinct rows."""
    hashes, ki, want = _batch_rows(nkeys, seed)
    idx = np.arange(n) % 96
    return hashes[idx].copy(), ki[idx].copy(), want[idx].copy()


# ---- DER: inputs whose signatures have the integer shapes the writer branches on ----
def der_fixture():
    """tests/golden/sign_der_cases.json: (hash, d) pairs found by signing
    seeded random pairs until r or s had a zero top byte, two zero top bytes,
    or the top bit set -- with the shortest and the longest encoding met."""
    with open(os.path.join(GOLDEN, "sign_der_cases.json")) as f:
        return json.load(f)["cases"]


def der_expected(rs_row) -> bytes:
    r, s = int.from_bytes(bytes(rs_row[:32]), "big"), int.from_bytes(bytes(rs_row[32:]), "big")
    return oder.encode(r, s)
