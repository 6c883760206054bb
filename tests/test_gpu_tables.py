"""The device table build (k_tab_bases / k_tab_small / k_tab_entries,
p256_kernels.hip) at its seams, through the public ABI: signatures with chosen
(u1, u2) (tests/tabgeom.py) whose signed digits read the first / last entry of
every H-row segment, phase-3 chunk, H row, window and phase-3 launch, the one
doubling entry m = 2 CL and its neighbours, in every window of the G table
(digit in u1) and of the first, a middle and the last key table (digit in u2),
with both signs.  Every accept bit is compared with the C oracle's; the CPU
harness builds its tables with other code (build_table_serial), so nothing
else aims at these kernels' entries.

A module of its own, one Verifier alive at a time: the (29, *) geometries hold
120 GB of HBM.  A geometry's tests share one context and one registration
(registering right after HBM was freed costs seconds).  The
library reads PBFTV_WAVE_MAX at pbftv_open and the binding forwards a changed
value before each verify, so the lane and the wave path run under the one
context."""
from __future__ import annotations

import numpy as np
import pytest

import tabgeom as tg

pytestmark = pytest.mark.gpu

# (G code, key code) -> registered keys.  All in kernels.h PBFTV_COMBOS; together every PBFTV_TABLE_WIDTHS entry.
GEOMETRIES = {
    (16, 12): 3,    # NH = 8: one H segment, clipped to 7
    (29, 21): 4,    # 36 G launches, narrow top windows in both tables: the production geometry
    (8, 8): 3,      # CL = kEnt = 128: no H rows, SEG < CL
    (16, 16): 130,  # NH = 128: two H segments (64 + 63); the 2^18-lane launch seam falls inside key 120
    (24, 20): 3,    # parts = 4
    (26, 22): 4,    # five G launches; the key launches meet inside key 2
    (29, 24): 2,    # 1.375 launches per key: a seam inside each key and a short last launch
}
# Geometries of the re-registration tests: the first entries of GEOMETRIES, in the same order (pytest groups a
# module-scoped parametrised fixture by parameter position, so these tests run while their geometry is open).
REBUILDS = [(16, 12), (29, 21)]
assert list(GEOMETRIES)[:len(REBUILDS)] == REBUILDS
_ID = "{0[0]}-{0[1]}".format


class Tables:
    """One open Verifier at one geometry, its key set, and the batches built for it."""

    def __init__(self, gq, oracle_lib):
        from simple_pbft_amd import Verifier
        self.gq, self.L = gq, oracle_lib
        self.rng = np.random.default_rng(gq[0] * 100 + gq[1])
        pairs = [tg.make_key(self.rng, oracle_lib) for _ in range(GEOMETRIES[gq])]
        if gq == (8, 8):  # key 0 = G here; a random key everywhere else
            from oracle import p256
            g = np.frombuffer(p256.GX.to_bytes(32, "big") + p256.GY.to_bytes(32, "big"), np.uint8)
            pairs[0] = (1, g.copy())
        self.base_privs = [d for d, _ in pairs]
        self.base_keys = np.stack([k for _, k in pairs])
        self.privs, self.keys = None, None
        self.cache = {}
        self.v = Verifier()

    def register(self, privs, keys, expect_valid=None):
        valid = self.v.register_keys(keys)
        assert self.v.table_config()[:2] == self.gq
        assert valid.tolist() == ([True] * len(keys) if expect_valid is None else expect_valid)
        self.privs, self.keys = list(privs), np.array(keys)

    def base(self):
        """The geometry's own key set, registered (again, if a test changed it)."""
        if self.keys is None or self.keys.shape != self.base_keys.shape or (self.keys != self.base_keys).any():
            self.register(self.base_privs, self.base_keys)
        return self


@pytest.fixture(scope="module", params=list(GEOMETRIES), ids=_ID)
def tab(request, oracle_lib):
    mp = pytest.MonkeyPatch()
    mp.setenv("PBFTV_GBITS", str(request.param[0]))
    mp.setenv("PBFTV_QBITS", str(request.param[1]))
    t = None
    try:
        t = Tables(request.param, oracle_lib)
        yield t
    finally:
        if t is not None:
            t.v.close()
        mp.undo()


@pytest.fixture(params=["lane", "wave"])
def path(request, monkeypatch):
    monkeypatch.setenv("PBFTV_WAVE_MAX", "100000000" if request.param == "wave" else "0")
    return request.param


def realised(code, probes, rng):
    """[(win, m)] -> both signs with a scalar each; asserts the drop rule.
    Returns [(win, m, sign, u)]."""
    g = tg.tabgeom(code)
    got, missing = [], []
    for win, m in probes:
        for sign in (1, -1):
            u = tg.scalar_with_digit(g.widths, win, sign * m, rng)
            (missing if u is None else got).append((win, m, sign, u))
    for win, m, sign, _ in missing:  # only -ent (not a digit) and top-window digits u < n excludes
        assert tg.may_be_missing(code, win, m, sign), (code, win, m, sign)
    assert len(got) + len(missing) == 2 * len(probes)
    # outside the top window exactly the -ent probes are missing
    assert sorted(p[:3] for p in missing if p[0] != g.kWin - 1) == sorted(
        (w, m, -1) for w, m in probes if w != g.kWin - 1 and m == g.ent(w))
    return got


def all_windows(code):
    return [(w, m) for w in range(tg.tabgeom(code).kWin) for m in tg.probe_multiples(code, w)]


def some_windows(code):
    """The reduced set: windows 0, the middle and the top one, all their multiples."""
    n = tg.tabgeom(code).kWin
    return [(w, m) for w in (0, n // 2, n - 1) for m in tg.probe_multiples(code, w)]


def make_batch(t, gprobes, kprobes):
    """One signature per pair (G-table probe in u1, key-table probe in u2), the
    shorter list cycled; every 8th signature again with r flipped.
    gprobes: [(win, m, sign, u)]; kprobes: [(key, win, m, sign, u)]."""
    assert gprobes and kprobes
    H, S, K, flip, names = [], [], [], [], []
    for i in range(max(len(gprobes), len(kprobes))):
        gw, gm, gs, u1 = gprobes[i % len(gprobes)]
        key, kw, km, ks, u2 = kprobes[i % len(kprobes)]
        for fl in ((False, True) if i % 8 == 0 else (False,)):
            h, rs = tg.chosen_scalar_sig_key(t.privs[key], u1, u2, fl, t.L)
            H.append(h)
            S.append(rs)
            K.append(key)
            flip.append(fl)
            names.append((("G", None, gw, gm, gs), ("key", key, kw, km, ks)))
    H, S, K, flip = np.stack(H), np.stack(S), np.array(K, np.uint32), np.array(flip)
    want = tg.oracle_bits(t.L, H, S, K, t.keys)
    # not vacuous: the oracle accepts every probe signature and rejects every twin
    assert want[~flip].all() and not want[flip].any()
    return H, S, K, flip, names, want


def check_batch(t, batch):
    H, S, K, flip, names, want = batch
    got = t.v.verify_batch(H, S, K)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d of %d bits differ from the oracle; (table, key, win, m, sign) of the first: %s" % (
        len(bad), len(K), [(names[i], "r flipped" if flip[i] else "accept expected") for i in bad[:20]])
    return len(K)


def probed_keys(t):
    """The first, a middle and the last key."""
    n = len(t.keys)
    return sorted({0, n // 2, n - 1})


def test_table_seams(tab, path):
    """Every probe multiple of every window, both signs, in the G table and in
    the first, a middle and the last key table; every bit against the oracle,
    through the lane and the wave path."""
    t = tab.base()
    if "seams" not in t.cache:
        gp = realised(t.gq[0], all_windows(t.gq[0]), t.rng)
        kp = [(key,) + p for key in probed_keys(t) for p in realised(t.gq[1], all_windows(t.gq[1]), t.rng)]
        t.cache["seams"] = make_batch(t, gp, kp)
    n = check_batch(t, t.cache["seams"])
    assert n >= 2 * len(all_windows(t.gq[1])) - tg.tabgeom(t.gq[1]).kWin


def test_table_slice_seams(tab, path):
    """The entries on both sides of every boundary between two phase-3
    launches, and the first and last entry of the last (shorter) launch, of the
    G build (one base) and of the key build (every registered key at once)."""
    t = tab.base()
    if "slices" not in t.cache:
        wg, wq = t.gq
        nk = len(t.keys)
        assert len(tg.slices(wg, 1)) == {8: 1, 16: 1, 24: 2, 26: 5, 29: 36}[wg]
        gs = tg.slice_seam_probes(wg, 1)
        ks = tg.slice_seam_probes(wq, nk)
        assert all(b == 0 for b, _, _ in gs) and all(b < nk for b, _, _ in ks)
        assert len(gs) >= 2 and len(ks) >= 2
        gp = realised(wg, sorted({(w, m) for _, w, m in gs}), t.rng)
        kp = []
        for key in sorted({b for b, _, _ in ks}):
            kp += [(key,) + p for p in realised(wq, sorted({(w, m) for b, w, m in ks if b == key}), t.rng)]
        t.cache["slices"] = make_batch(t, gp, kp)
    check_batch(t, t.cache["slices"])


def reduced_batch(t, keys):
    gp = realised(t.gq[0], some_windows(t.gq[0]), t.rng)
    kp = [(key,) + p for key in keys for p in realised(t.gq[1], some_windows(t.gq[1]), t.rng)]
    return make_batch(t, gp, kp)


def stale_batch(t, priv, key):
    """Probe signatures made with the private scalar `priv`, naming key `key`: (H, S, K)."""
    gp = realised(t.gq[0], [(0, 1), (0, 2)], t.rng)
    kp = realised(t.gq[1], [(w, m) for w in range(tg.tabgeom(t.gq[1]).kWin - 1) for m in (1, 2)], t.rng)
    sigs = [tg.chosen_scalar_sig_key(priv, gp[i % len(gp)][3], p[3], False, t.L) for i, p in enumerate(kp)]
    return np.stack([h for h, _ in sigs]), np.stack([rs for _, rs in sigs]), np.full(len(sigs), key, np.uint32)


@pytest.mark.parametrize("tab", REBUILDS, indirect=True, ids=_ID)
def test_tables_beside_an_invalid_key(tab):
    """An off-curve key in the middle of a registration: k_tab_bases reports it
    invalid and builds a stand-in table in its slot; every signature naming it
    is rejected, and the tables on both sides of it are whole."""
    t = tab
    privs, keys = list(t.base_privs), t.base_keys.copy()
    bad = len(keys) // 2
    keys[bad, 40] ^= 0x10  # y off the curve
    assert t.L.oracle_p256_key_valid(keys[bad].ctypes.data) == 0
    t.register(privs, keys, [k != bad for k in range(len(keys))])
    H, S, K, flip, names, want = reduced_batch(t, [bad - 1, bad + 1])
    check_batch(t, (H, S, K, flip, names, want))
    # the neighbours' signatures, and ones made with the private scalar of the key it was, under the invalid key
    assert not t.v.verify_batch(H, S, np.full_like(K, bad)).any()
    H, S, K = stale_batch(t, privs[bad], bad)
    assert not tg.oracle_bits(t.L, H, S, K, keys).any()
    assert tg.oracle_bits(t.L, H, S, K, t.base_keys).all()  # good signatures for the key before it was bent
    assert not t.v.verify_batch(H, S, K).any()


@pytest.mark.parametrize("tab", REBUILDS, indirect=True, ids=_ID)
def test_tables_after_add_and_set_key(tab):
    """Builds with key0 != 0 (pbftv_add_keys, pbftv_set_key: launch-relative
    key indexing): the replaced key's, both added keys' and an untouched key's
    tables are whole, and signatures for the replaced key's old private scalar
    are rejected."""
    t = tab
    extra = [tg.make_key(t.rng, t.L) for _ in range(3)]
    privs, keys = list(t.base_privs[:3]), t.base_keys[:3].copy()
    t.register(privs, keys)
    assert t.v.add_keys(np.stack([extra[0][1], extra[1][1]])).tolist() == [True, True]
    assert t.v.set_key(1, extra[2][1]) is True
    t.privs = [privs[0], extra[2][0], privs[2], extra[0][0], extra[1][0]]
    t.keys = np.stack([keys[0], extra[2][1], keys[2], extra[0][1], extra[1][1]])
    assert t.v.table_config()[:2] == t.gq
    check_batch(t, reduced_batch(t, [1, 3, 4, 2]))
    H, S, K = stale_batch(t, privs[1], 1)
    assert tg.oracle_bits(t.L, H, S, K, keys).all()  # good signatures for the key that was replaced
    assert not tg.oracle_bits(t.L, H, S, K, t.keys).any()
    assert not t.v.verify_batch(H, S, K).any()
