"""Every on-device inversion mod n on chosen inputs (tests/scalar_cases.py).

w = s^-1 mod n is the one piece of ECDSA arithmetic here with no host build:
inv_mod_n_wave (verify_kernels.h: one 30-bit limb per lane, divsteps in
hand-scheduled scalar assembly) behind wave_scalars / wave_scalars_lds on the
latency path, and behind wave_batch_inv_n / block_batch_inv_n in the lane
path's k_ecdsa_scalars<K>.  Each signature here is VALID for a chosen s (the
hash is solved for), so a wrong inverse turns an expected 1 into a 0; each has
a twin (r xor 2) that must stay 0.  Expected bits are the C oracle's; that the
valid ones expect 1 and the twins 0 is asserted too.  Every comparison is
exact, a bit per signature.

Which kernel serves which phase (read from launch_wave_w / launch_armed_w;
pbftv_qc_counters confirms launched vs armed).  The row schedule exists for 9
to 16 windows only (RowsGeom::ok), and 16-bit windows make 17: at (16, 16) --
the cheapest geometry, used wherever it can be -- a certificate is served by
the one-wave kernels, which call wave_scalars.  The row kernels, which call
wave_scalars_lds, get the cheapest geometry that has them, (20, 20).

  phase      geometry  environment                   kernel
  quad       (16, 16)  PBFTV_QC_ROWS=0, calls <= 128  k_ecdsa_wave
  lean       (16, 16)  PBFTV_QC_BUSY_ONE_WAVE=2      k_ecdsa_wave_lean
  wide       (16, 16)  two calls of 1144 (129..2048)  k_ecdsa_wave (every geometry:
                                                      rows_max_batch() is 128)
  rows       (20, 20)  calls <= 128                  k_ecdsa_rows
  armed      (16, 16)  certificates of 4 / of 67     k_ecdsa_wave_armed, 8 slots / 128
  armed      (20, 20)  certificates of 4 / of 67     k_ecdsa_rows_armed, narrow / wide

The lane path runs groups(K) (chosen totals for the shared inversions, members
at every j and at the lanes 0, 63, 64, 255) for K = 1, 2, 4, 8, 16 under 12
keys, without the key order and -- K = 4 and 16, where kstart first serves the
key order and then holds block_batch_inv_n's slots -- with it.  The free-key
grid (e at and beyond n, x_R at the seams of r + n < p and of [n, p)) goes
through the verify that carries keys, in X||Y and compressed form, and through
both registered paths at (16, 8).

That the module bites was shown once with three one-line experiment builds
(never committed), each failing exactly where tests/safegcd_model.py and
scalar_cases.ownership() predicted, signature for signature:
  * inv_mod_n_wave's fix-up "+ 16 n" as "+ 0 n": all 16 tests fail; of the
    first 64 S_EDGE values those with a negative final d fail (n - 1, n - 3,
    (n - 1) / 2, 2^6) -- but not n - 2: the device then uses w + 1, the sum
    becomes (1 + s) k G = -k G, and its x is still r;
  * an out-of-range s joining the lane's product as 2: the lane tests fail for
    K >= 2 only, at the 20 / 60 / 184 / 390 valid signatures that share a lane
    with such a member at a higher j (or with the ragged tail);
  * block_batch_inv_n's select for a quad's last lane taking the prefix: the
    lane tests fail for K >= 4 only, at every valid signature of lanes 3 mod 4
    except in the all-ones block."""
from __future__ import annotations

import time

import numpy as np
import pytest

import scalar_cases as sc
import wirekey_cases as wc

pytestmark = pytest.mark.gpu

_COUNTERS = ("calls", "armed", "reruns", "exact_sigs", "launches")


@pytest.fixture(scope="module")
def edge(oracle_lib):
    """S_EDGE signatures and twins under fixed key 0 with the oracle's bits"""
    es = sc.edge_signatures()
    want = sc.oracle_keyed(oracle_lib, es["hashes"], es["sigs"], sc.fixed_keys()[1], es["kidx"])
    assert want[es["valid"]].all() and not want[~es["valid"]].any() and es["valid"].sum() >= 1100
    return es["hashes"], es["sigs"], es["kidx"], want, es["labels"]


@pytest.fixture(scope="module")
def grid(oracle_lib):
    g = sc.grid()
    want = sc.oracle_own_key(oracle_lib, g["hashes"], g["sigs"], g["pubs"])
    assert want[g["valid"]].all() and not want[~g["valid"]].any() and g["valid"].sum() == 324
    return g, want


_group_expect: dict = {}


def _groups(oracle_lib, K):
    """groups(K) with the oracle's bits, computed once per K"""
    if K not in _group_expect:
        G = sc.groups(K)
        want = sc.oracle_keyed(oracle_lib, G["hashes"], G["sigs"], sc.fixed_keys()[1], G["kidx"])
        assert want[G["valid"]].all() and not want[~G["valid"]].any()
        _group_expect[K] = (G, want)
    return _group_expect[K]


def _open(monkeypatch, gq, keys, **env):
    from simple_pbft_amd import Verifier
    monkeypatch.setenv("PBFTV_GBITS", str(gq[0]))
    monkeypatch.setenv("PBFTV_QBITS", str(gq[1]))
    for k in ("PBFTV_WAVE_MAX", "PBFTV_QC_ROWS", "PBFTV_QC_BUSY_ONE_WAVE", "PBFTV_QC_WIDE", "PBFTV_QC_ROWS_MAX",
              "PBFTV_QC_SLOTS", "PBFTV_SCALAR_BATCH", "PBFTV_KEY_SORT", "PBFTV_HOST_CHUNK", "PBFTV_ALIAS_DEVICES"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    v = Verifier(device_mask=1)
    assert v.register_keys(keys).all()
    assert v.table_config()[:2] == gq
    return v


def _call(v, data, idx):
    """one verify_batch of rows idx: every bit against the oracle's; the counters' change"""
    H, S, K, want, labels = data
    c0 = v.qc_counters(0)
    got = v.verify_batch(H[idx], S[idx], K[idx])
    c1 = v.qc_counters(0)
    bad = [labels[idx[i]] for i in np.nonzero(got != want[idx])[0]]
    assert not bad, bad[:12]
    return {k: c1[k] - c0[k] for k in _COUNTERS}


def _wait_armed(v, data, idx, wide: bool, limit_s: float = 5.0):
    """certificates until one is served by the armed kernel of the right shape
    (the keeper arms after the first call; a wide kernel needs all of its
    workgroups resident)"""
    t0 = time.monotonic()
    while time.monotonic() - t0 < limit_s:
        d = _call(v, data, idx)
        c = v.qc_counters(0)
        if d["armed"] == 1 and c["armed_wide"] == wide:
            return
        time.sleep(0.01)
    raise AssertionError(f"no armed {'wide' if wide else 'narrow'} kernel within {limit_s} s: {v.qc_counters(0)}")


LAUNCHED = {
    "quad": ((16, 16), {"PBFTV_QC_ROWS": "0"}, 128),
    "lean": ((16, 16), {"PBFTV_QC_BUSY_ONE_WAVE": "2"}, 128),
    "wide": ((16, 16), {}, 1144),
    "rows": ((20, 20), {}, 128),
}


@pytest.mark.parametrize("phase", list(LAUNCHED))
def test_latency_launched_kernels(phase, edge, monkeypatch):
    """S_EDGE and twins through each launched latency kernel (the module
    docstring's table): one launch per call, none armed."""
    gq, env, per = LAUNCHED[phase]
    n = len(edge[3])
    with _open(monkeypatch, gq, sc.fixed_keys()[1][:1], PBFTV_QC_ARM="0", **env) as v:
        for a in range(0, n, per):
            d = _call(v, edge, np.arange(a, min(a + per, n)))
            assert (d["calls"], d["armed"], d["launches"]) == (1, 0, 1), (phase, a, d)


@pytest.mark.parametrize("gq", [(16, 16), (20, 20)])
def test_latency_armed_kernels(gq, edge, monkeypatch):
    """S_EDGE and twins through the armed kernels: certificates of 4 (narrow)
    and of 67 (wide; consecutive signatures, so the edge values sit at slot and
    at helper positions alike).  Every call is served armed; one that the row
    schedule hands back (result byte 2) is rerun by a launch, nothing is
    asserted on how many."""
    n = len(edge[3])
    plain = np.arange(0, 8, 2)  # four valid signatures
    with _open(monkeypatch, gq, sc.fixed_keys()[1][:1], PBFTV_QC_ARM="1", PBFTV_QC_ARM_MS="30000",
               PBFTV_QC_WIDE="0") as v:
        _wait_armed(v, edge, plain, wide=False)
        for a in range(0, n, 4):
            d = _call(v, edge, np.arange(a, min(a + 4, n)))
            assert (d["calls"], d["armed"]) == (1, 1), (a, d)
        monkeypatch.delenv("PBFTV_QC_WIDE")
        _wait_armed(v, edge, np.arange(0, 134, 2), wide=True)  # (the first wide call is launched, the next arming is wide)
        for a in range(0, n, 67):
            d = _call(v, edge, np.arange(a, a + 67) % n)
            assert (d["calls"], d["armed"]) == (1, 1), (a, d)
        assert v.qc_counters(0)["armed_wide"]


@pytest.mark.parametrize("K,sort", [(1, "0"), (2, "0"), (4, "0"), (8, "0"), (16, "0"), (4, "1"), (16, "1")])
def test_lane_path_chosen_totals(K, sort, oracle_lib, monkeypatch):
    """groups(K) through k_ecdsa_scalars<K>: every wave's (K <= 2) or block's
    (K >= 4) shared inversion receives a chosen total."""
    G, want = _groups(oracle_lib, K)
    with _open(monkeypatch, (16, 16), sc.fixed_keys()[1], PBFTV_WAVE_MAX="0", PBFTV_SCALAR_BATCH=str(K),
               PBFTV_KEY_SORT=sort) as v:
        got = v.verify_batch(G["hashes"], G["sigs"], G["kidx"])
    bad = np.nonzero(got != want)[0]
    owner = sc.ownership(K, G["n"])
    assert not len(bad), [(int(i), G["kind"][i], "lane %d j %d group %d" % tuple(int(o[i]) for o in owner[1:]))
                          for i in bad[:12]]


def test_grid_with_carried_keys(grid):
    """the 324 free-key triples and their twins, the key riding with the signature"""
    from simple_pbft_amd import Verifier
    g, want = grid
    with Verifier(device_mask=1) as v:
        got = v.verify_pubkey_batch(g["hashes"], g["sigs"], g["pubs"])
        assert (got == want).all(), [g["labels"][i] for i in np.nonzero(got != want)[0][:12]]
        comp = wc.encode(g["pubs"], wc.KEY_COMPRESSED)
        assert (wc.decoded_xy(comp, wc.KEY_COMPRESSED)[0] == g["pubs"]).all()
        got = v.verify_wirekey_batch(g["hashes"], g["sigs"], comp, wc.KEY_COMPRESSED)
        assert (got == want).all(), [g["labels"][i] for i in np.nonzero(got != want)[0][:12]]


@pytest.mark.parametrize("path", ["lane", "latency"])
def test_grid_with_registered_keys(path, grid, monkeypatch):
    """the same under its 324 registered keys at (16, 8): the lane path in one
    batch, the latency path in calls of at most 128"""
    g, want = grid
    keys, kidx = sc.grid_registered()
    data = (g["hashes"], g["sigs"], kidx, want, g["labels"])
    n = len(want)
    env = {"PBFTV_WAVE_MAX": "0"} if path == "lane" else {"PBFTV_QC_ARM": "0"}
    with _open(monkeypatch, (16, 8), keys, **env) as v:
        for a in range(0, n, n if path == "lane" else 128):
            d = _call(v, data, np.arange(a, min(a + 128, n) if path == "latency" else n))
            assert d["launches"] == (0 if path == "lane" else 1), d
