"""The comb on the column-order field products (fes.h fs_mul and its kin, the
paired forms in xyzz_madd_s_flip / xyzz_aff_aff_s / xyzz_last_prep_s), small
lane-path batches, every bit against the C oracle:

  * 4,096 oracle-signed signatures over 12 keys, key order on, 1 % corrupted
    across the usual 8 classes;
  * tests/golden/ecdsa.json, every geometry's list of
    tests/golden/rows_exceptional.json and conftest's crafted doubling /
    cancellation sums (key 0 = G), padded to 4,096 with the golden vectors
    again: the first-pair path, the fused last step and the complete-addition
    rerun in waves that run the new products;

at a small geometry (8, 8) and the mixed one (29, 21), both among
test_gpu_geometry.py's.  The table builder runs on the same products
(registration, here and in test_gpu_tables.py)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import rowtree
from conftest import GOLDEN, crafted_exceptional, fixture_arrays, oracle_sign_pool
from test_gpu_key_order import corrupt

pytestmark = pytest.mark.gpu

BATCH = 4096
GEOMETRIES = [(8, 8), (29, 21)]


@pytest.fixture(scope="module")
def signed(oracle_lib):
    keys, H, S, K = oracle_sign_pool(oracle_lib, n_keys=12, per_key=342, seed=0xF5C0)
    rng = np.random.default_rng(0xF5C1)
    pick = rng.permutation(len(K))[:BATCH]
    H, S, K = H[pick].copy(), S[pick].copy(), K[pick].copy()
    corrupt(H, S, K, 12, 0.01, rng)  # 1 % (41), the usual 8 classes
    want = _oracle(oracle_lib, keys, H, S, K)
    assert want.sum() == BATCH - 41
    return keys, H, S, K, want


@pytest.fixture(scope="module")
def golden(oracle_lib, ecdsa_fixtures):
    gkeys, H, S, K, E = fixture_arrays(ecdsa_fixtures)
    keys = np.concatenate([rowtree.g_key(), gkeys])  # key 0 is G, the golden keys follow
    H, S, K, E = list(H), list(S), list(K + 1), list(E)
    n_golden = len(K)
    with open(os.path.join(GOLDEN, "rows_exceptional.json")) as f:
        geoms = json.load(f)["geometries"]
    for name in sorted(geoms):
        for v in geoms[name]:
            H.append(np.frombuffer(bytes.fromhex(v["hash"]), np.uint8))
            S.append(np.frombuffer(bytes.fromhex(v["r"]) + bytes.fromhex(v["s"]), np.uint8))
            K.append(0)
            E.append(bool(v["expect"]))
    _, H2, S2, K2, E2 = crafted_exceptional()
    H, S, K, E = H + list(H2), S + list(S2), K + [0] * len(K2), E + [bool(e) for e in E2]
    assert len(K) <= BATCH
    for j in range(BATCH - len(K)):  # padding: the golden vectors again
        H.append(H[j % n_golden]), S.append(S[j % n_golden]), K.append(K[j % n_golden]), E.append(E[j % n_golden])
    H, S, K = np.stack(H), np.stack(S), np.array(K, np.uint32)
    want = _oracle(oracle_lib, keys, H, S, K)
    assert (want == np.array(E, bool)).all()  # the fixtures' own expectations are the oracle's
    return keys, H, S, K, want


def _oracle(oracle_lib, keys, H, S, K):
    n = len(K)
    bm = np.zeros((n + 7) // 8, np.uint8)
    keys, H, S, K = (np.ascontiguousarray(a) for a in (keys, H, S, K))
    oracle_lib.oracle_ecdsa_p256_verify_batch(H.ctypes.data, S.ctypes.data, K.ctypes.data, n, keys.ctypes.data,
                                              len(keys), bm.ctypes.data, 16)
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


def _run(gq, monkeypatch, batch):
    from simple_pbft_amd import Verifier
    monkeypatch.setenv("PBFTV_GBITS", str(gq[0]))
    monkeypatch.setenv("PBFTV_QBITS", str(gq[1]))
    monkeypatch.setenv("PBFTV_WAVE_MAX", "0")   # the lane path (k_ecdsa_comb) at this size
    monkeypatch.setenv("PBFTV_KEY_SORT", "1")   # the key order below the default rule's 32k
    keys, H, S, K, want = batch
    with Verifier(device_mask=1) as v:
        v.register_keys(keys)
        assert v.table_config()[:2] == gq
        before = v.lib_counters(0)["sorted_batches"]
        got = v.verify_batch(H, S, K)
        assert v.lib_counters(0)["sorted_batches"] - before >= 1  # the key order was taken
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, (len(diff), diff[:10])


@pytest.mark.parametrize("gq", GEOMETRIES)
def test_signed_batch_over_12_keys(gq, signed, monkeypatch):
    _run(gq, monkeypatch, signed)


@pytest.mark.parametrize("gq", GEOMETRIES)
def test_golden_and_exceptional_vectors(gq, golden, monkeypatch):
    _run(gq, monkeypatch, golden)
