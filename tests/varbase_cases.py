"""Inputs for the verify under unregistered keys (simple_pbft_amd/csrc/varbase.h),
shared by tests/test_varbase_cpu.py and tests/test_gpu_varbase.py.  Every
expected bit comes from the oracle (oracle_ecdsa_p256_verify, which rejects a
key that oracle_p256_key_valid rejects); each set is computed once."""
from __future__ import annotations

import json
import os

import numpy as np

from conftest import GOLDEN, chosen_scalar_sig, crafted_exceptional, fixture_arrays, oracle_sign_pool

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551

_cache: dict = {}


def oracle_expect(oracle_lib, hashes, sigs, pubs) -> np.ndarray:
    """oracle_ecdsa_p256_verify of signature i under pubs[i], one by one."""
    hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
    sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 64)
    pubs = np.ascontiguousarray(pubs, np.uint8).reshape(-1, 64)
    out = np.zeros(len(hashes), bool)
    for i in range(len(hashes)):
        ok = oracle_lib.oracle_ecdsa_p256_verify(hashes[i].ctypes.data, sigs[i].ctypes.data, pubs[i].ctypes.data)
        assert ok == 0 or oracle_lib.oracle_p256_key_valid(pubs[i].ctypes.data) == 1
        out[i] = ok == 1
    return out


def oracle_expect_keyed(oracle_lib, hashes, sigs, keys, kidx) -> np.ndarray:
    """The same through the oracle's batch form (threads) over a key table."""
    n = len(kidx)
    hashes, sigs = np.ascontiguousarray(hashes, np.uint8), np.ascontiguousarray(sigs, np.uint8)
    keys, kidx = np.ascontiguousarray(keys, np.uint8), np.ascontiguousarray(kidx, np.uint32)
    bm = np.zeros((n + 7) // 8, np.uint8)
    oracle_lib.oracle_ecdsa_p256_verify_batch(hashes.ctypes.data, sigs.ctypes.data, kidx.ctypes.data, n,
                                              keys.ctypes.data, len(keys), bm.ctypes.data, 8)
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


def _g_key():
    from oracle import p256
    return np.frombuffer(p256.GX.to_bytes(32, "big") + p256.GY.to_bytes(32, "big"), np.uint8)


# (name, u1, u2, the exact rerun must run) under the key Q = G
def crafted_scalars():
    a, b, c, m = 5, 9, 3, 77
    u1_plain = 0x1234567
    out = []
    for u2 in (1, 2, 7, 8, 9, 15, 16, 17, 1 << 128, N - 1, int("8" * 64, 16), int("9" * 64, 16)):
        out.append(("ladder u2=%x" % u2, u1_plain, u2, False))
    # the one scalar whose LAST ladder step is a doubling modulo n (varbase.h)
    out.append(("ladder u2=n-2", u1_plain, N - 2, True))
    for i in (0, 8, 15):
        out.append(("doubling at G window %d" % i, m << (16 * i), m << (16 * i), True))
    out.append(("final cancellation", 0xABCDEF << 64, N - (0xABCDEF << 64), True))
    out.append(("mid-sum doubling", a + (b << 16), (b << 16) - a, True))
    out.append(("mid-sum cancellation, continues from infinity", a + (b << 16) + (c << 32),
                (-(b << 16) - a) % N, True))
    return out


def crafted_set(oracle_lib):
    """hashes, sigs, pubs, expect, names, rerun (None: not pinned) -- every
    chosen-scalar signature with its r-flipped twin, then the key cases."""
    if "crafted" in _cache:
        return _cache["crafted"]
    g = _g_key()
    H, S, K, names, rerun = [], [], [], [], []
    for name, u1, u2, rr in crafted_scalars():
        for flip in (False, True):
            h, rs, want = chosen_scalar_sig(u1, u2, flip)
            H.append(h)
            S.append(rs)
            K.append(g)
            names.append(name + (" (r flipped)" if flip else ""))
            rerun.append(None if flip else rr)  # (a flipped r changes u2: other scalars, nothing pinned)
            got = oracle_lib.oracle_ecdsa_p256_verify(h.ctypes.data, rs.ctypes.data, g.ctypes.data)
            assert bool(got) == bool(want), name
    # keys: a valid signature, then the same under broken keys
    keys, hashes, sigs, kidx = oracle_sign_pool(oracle_lib, 2, 1, seed=4242)
    x = int.from_bytes(keys[0, :32].tobytes(), "big")
    y = int.from_bytes(keys[0, 32:].tobytes(), "big")

    def key(xx, yy):
        return np.frombuffer(xx.to_bytes(32, "big") + yy.to_bytes(32, "big"), np.uint8)

    for name, k in (("valid key", keys[0]), ("off-curve key", key(x, (y + 1) % P)), ("x = p", key(P, y)),
                    ("y >= p", key(x, (1 << 256) - 1)), ("y = p", key(x, P)), ("key (0, 0)", key(0, 0)),
                    ("valid key, y negated", key(x, P - y)), ("another valid key", keys[1])):
        H.append(hashes[0])
        S.append(sigs[0])
        K.append(np.array(k, np.uint8))
        names.append(name)
        rerun.append(None)
    H, S, K = np.stack(H), np.stack(S), np.stack(K)
    expect = oracle_expect(oracle_lib, H, S, K)
    assert expect[names.index("valid key")] and not expect[names.index("valid key, y negated")]
    _cache["crafted"] = (H, S, K, expect, names, rerun)
    return _cache["crafted"]


def golden_set(oracle_lib):
    """The 163 golden vectors with the key taken from the fixture.  A vector
    whose key index lies outside the fixture's key list (rejected there for
    that reason) has no key to carry: it gets the all-zero key, which is not a
    point of the curve, and stays a rejection."""
    if "golden" in _cache:
        return _cache["golden"]
    with open(os.path.join(GOLDEN, "ecdsa.json")) as f:
        fx = json.load(f)
    keys, hashes, sigs, kidx, expect = fixture_arrays(fx)
    pubs = np.zeros((len(kidx), 64), np.uint8)
    inside = kidx < len(keys)
    pubs[inside] = keys[kidx[inside]]
    assert not expect[~inside].any()
    want = oracle_expect(oracle_lib, hashes, sigs, pubs)
    assert (want == expect).all()
    _cache["golden"] = (hashes, sigs, np.ascontiguousarray(pubs), want)
    return _cache["golden"]


def exceptional_set(oracle_lib):
    """conftest.crafted_exceptional() (key Q = G)."""
    if "exc" in _cache:
        return _cache["exc"]
    key, H, S, K, E = crafted_exceptional()
    pubs = np.ascontiguousarray(key[K])
    want = oracle_expect(oracle_lib, H, S, pubs)
    assert (want == E).all()
    _cache["exc"] = (H, S, pubs, want)
    return _cache["exc"]


def all_vectors(oracle_lib):
    """golden + crafted_exceptional + crafted set, concatenated: hashes, sigs, pubs, expect."""
    if "all" in _cache:
        return _cache["all"]
    g, e, c = golden_set(oracle_lib), exceptional_set(oracle_lib), crafted_set(oracle_lib)
    _cache["all"] = tuple(np.ascontiguousarray(np.concatenate([g[k], e[k], c[k]])) for k in range(4))
    return _cache["all"]


def random_signed(oracle_lib, n_keys, per_key, seed, corrupt, corrupt_keys=True):
    """Oracle-signed signatures over n_keys keys in shuffled order, a fraction
    `corrupt` of them with one bit flipped in the hash, r, s or (corrupt_keys) the key:
    keys, hashes, sigs, kidx, pubs (the possibly corrupted key of each), corrupted mask."""
    keys, hashes, sigs, kidx = oracle_sign_pool(oracle_lib, n_keys, per_key, seed)
    rng = np.random.default_rng(seed + 1)
    n = len(kidx)
    perm = rng.permutation(n)
    hashes, sigs, kidx = hashes[perm].copy(), sigs[perm].copy(), kidx[perm].copy()
    pubs = keys[kidx].copy()
    bad = np.zeros(n, bool)
    for i in rng.choice(n, max(1, int(n * corrupt)), replace=False):
        what = int(rng.integers(0, 4 if corrupt_keys else 3))
        arr = (hashes, sigs, sigs, pubs)[what]
        lo, hi = ((0, 32), (0, 32), (32, 64), (0, 64))[what]
        arr[i, int(rng.integers(lo, hi))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        bad[i] = True
    return keys, hashes, sigs, kidx, pubs, bad
