"""tests/rowfield.py -- the limb-exact model of rows.h and of the quad schedule
-- against plain Python integers, over the families of tests/rowfield_cases.py
(the ones tests/test_gpu_field_probe.py puts to the device), with the coverage
those families must reach asserted in code, and the model's teeth."""
from __future__ import annotations

import numpy as np
import pytest

import rowfield as rf
import rowfield_cases as rc
from rowfield_suite import row_suite
from rowfield_cases import P, RINV
from test_algo_cpu import H  # noqa: F401  (the CPU harness, rebuilt when stale)

N_WAVES = 1024


@pytest.fixture(scope="module")
def suite():
    return row_suite(N_WAVES)


def _plain(x):
    return rc.plain(x)


def test_row_mul_is_the_montgomery_product(suite):
    """every product equals a b 2^-261 mod p, |value| < |a| |b| / 2^261 + p"""
    c = suite["row_mul"]
    a, b, o = rc.values(c["a"]), rc.values(c["b"]), rc.values(c["out"])
    assert len(o) == 4 * N_WAVES
    for x, y, v in zip(a, b, o):
        assert v % P == x * y * RINV % P
        assert abs(v) * rc.R < abs(x * y) + P * rc.R


def test_row_norm_keeps_the_value(suite):
    c = suite["row_norm"]
    assert rc.values(c["x"]) == rc.values(c["out"])


def test_coverage_of_the_families(suite):
    """The bounds of rows.h's header are REACHED, not only respected: the widest
    pair drives max|a_i| max|b_j| to 2^60.9 and the columns past 2^61 (below
    the stated 2^61.2), the final carries take both signs, and every limb
    position of either operand slot is seen at both bounds of its type."""
    st = suite["model"].stats
    assert st["prod"] >= 2 ** 60.9 and st["prod"] < rf.PROD_BOUND
    assert st["col"] >= 2 ** 61 and st["col"] < rf.COL_BOUND
    assert st["carry_min"] < 0 < st["carry_max"]
    assert st["limb_min"] < 0 and st["limb_max"] >= 1 << 29
    c = suite["row_mul"]
    flat = {"a": c["a"].reshape(-1, 16)[:, :9], "b": c["b"].reshape(-1, 16)[:, :9]}
    for slot, k in (("a", 0), ("b", 1)):
        for typ in sorted({t[k] for t in c["types"]}):
            rows = flat[slot][[i for i, t in enumerate(c["types"]) if t[k] == typ]]
            lo, hi = rc.box(typ)
            assert ((rows == hi).any(axis=0) & (rows == lo).any(axis=0)).all(), (slot, typ)
            assert rc.in_type(rows, typ)


def test_xyzz_add_rows_is_add_2008_s(suite):
    c = suite["add"]
    A, B = [_plain(c["A"][:, k]) for k in range(4)], [_plain(c["B"][:, k]) for k in range(4)]
    rm = _plain(c["rm"])
    out = [_plain(v[:, 0]) for v in c["out"]]
    rz = _plain(c["rz"][:, 0])
    for i in range(N_WAVES):
        want, wrz = rc.add_formula([A[k][i] for k in range(4)], [B[k][i] for k in range(4)], rm[i])
        assert [out[k][i] for k in range(4)] == want and rz[i] == wrz, c["labels"][i]
        if c["labels"][i] in ("double", "cancel", "zz0"):
            assert out[2][i] == 0 and out[3][i] == 0  # ZZ3 == ZZZ3 == 0 comes out
    for v in c["out"] + [c["rz"]]:  # the sum is the same in every row
        assert (v == v[:, :1]).all()


def test_xyzz_add_rows_on_curve_points(suite):
    """iv: with real points the XYZZ sum is the curve's sum"""
    from oracle import p256
    c = suite["add"]
    idx = [i for i, l in enumerate(c["labels"]) if l == "curve"]
    assert len(idx) >= 32
    pts = rc.curve_points(2 * len(idx), 11)
    out = [_plain(v[idx, 0]) for v in c["out"]]
    for j in range(len(idx)):
        x, y = p256.point_add(pts[j], pts[len(idx) + j])
        zz, zzz = out[2][j], out[3][j]
        assert out[0][j] == x * zz % P and out[1][j] == y * zzz % P and zz * zz * zz % P == zzz * zzz % P


def test_mmadd_pairs_is_mmadd_2008_s(suite):
    c = suite["mmadd"]
    ins = [_plain(v[:, 0::2].reshape(-1, 16)) for v in c["ins"]]
    out = [_plain(v[:, 0::2].reshape(-1, 16)) for v in c["out"]]
    for i in range(2 * N_WAVES):
        assert [o[i] for o in out] == rc.mmadd_formula(*[v[i] for v in ins]), c["labels"][i]
        if c["labels"][i] in ("double", "cancel"):
            assert out[2][i] == 0 and out[3][i] == 0
    for v in c["out"]:  # both rows of a pair hold the pair's sum
        assert (v[:, 0] == v[:, 1]).all() and (v[:, 2] == v[:, 3]).all()


def test_chain_of_four_levels(suite):
    """outputs feed inputs: the top of each tree is the sum of its 16 leaves,
    and a doubling or cancellation at level 1 leaves ZZ == 0 at every level above"""
    from oracle import p256
    c = suite["chain"]
    n = c["chains"]
    for lv, L in enumerate(c["levels"]):
        zz = np.array([v == 0 for v in _plain(L["out"][2][:, 0])]).reshape(n, -1)
        assert not zz[:2].any()
        assert zz[2:, 0].all() and not zz[2:, 1:].any()
        A = [_plain(v[:, 0]) for v in L["A"]]
        B = [_plain(v[:, 0]) for v in L["B"]]
        out = [_plain(v[:, 0]) for v in L["out"]]
        for i in range(len(out[0])):
            assert [o[i] for o in out] == rc.add_formula([a[i] for a in A], [b[i] for b in B])[0]
    top = [_plain(v[:, 0]) for v in c["levels"][3]["out"]]
    for ch in range(2):
        acc = None
        for pt in c["points"][16 * ch:16 * ch + 16]:
            acc = pt if acc is None else p256.point_add(acc, pt)
        assert top[0][ch] == acc[0] * top[2][ch] % P and top[1][ch] == acc[1] * top[3][ch] % P


def test_fused_check_verdict_and_exc(suite):
    """the verdict is X3 == r ZZ3 and exc is P == 0 or r ZZ1 ZZ2 == 0, on the
    crafted cases (accept, r ^ 2, P == 0, a zero ZZ) and on the families"""
    c = suite["check"]
    A, B = [_plain(c["A"][:, k]) for k in range(4)], [_plain(c["B"][:, k]) for k in range(4)]
    rz = _plain(c["rz"])
    seen = set()
    for i in range(len(rz)):
        ok, exc = rc.check_formula([a[i] for a in A], [b[i] for b in B], rz[i])
        assert (bool(c["ok"][i]), bool(c["exc"][i])) == (ok, exc), i
        if i < len(c["want"]):
            w_ok, w_exc = c["want"][i]
            assert exc == w_exc and (exc or ok == w_ok), i
            seen.add((ok, exc))
    assert {(True, False), (False, False), (False, True)} <= seen  # both ballot halves, both ways


def test_row_is_zero(suite):
    c = suite["zero"]
    want = [v % P == 0 for v in rc.values(c["x"][:, 0])]
    assert list(c["out"]) == want and 20 <= sum(want) < len(want)


def test_row_entry_unpacks_the_table():
    tab = rc.entry_table()
    for d in list(range(-len(tab), len(tab) + 1)):
        e = tab[max(abs(d) - 1, 0)]
        x = sum(int(w) << (32 * i) for i, w in enumerate(e[:8]))
        y = sum(int(w) << (32 * i) for i, w in enumerate(e[8:]))
        got = [rf.row_entry(tab, d, L) for L in range(16)]
        assert rc.val([g[0] for g in got[:9]]) == x and rc.val([g[1] for g in got[:9]]) == y
        assert all(g[0] < (1 << 29) and g[1] < (1 << 29) for g in got[:8]) and got[9:] == [(0, 0)] * 7


# ---- teeth -----------------------------------------------------------------------
def _po_bounds(rng, n):
    return rc.uniform_wave(rc.bound_family(rng, "PO", n))


def test_teeth_x3_without_its_row_norm():
    """X3 = R^2 - PPP - 2Q un-normalised makes Q - X3 = 3Q + PPP - R^2 leave int32
    -- but only with three product limbs at their extremes at once (Q and PPP
    at the upper bound where R^2 is at the lower).  R^2, PPP and Q are product
    OUTPUTS: no choice of an addition's inputs steers three of them there, so
    the bound family meets the step itself (RowModel.x3_step, the two lines
    xyzz_add_rows and mmadd_pairs share).  The mutant trips the int32
    assertion there; the real step does not; and 10,000 random additions
    through the whole mutant never trip it -- random inputs do not reach what
    the families reach."""
    rng = np.random.default_rng(5)
    n = 64
    Q, PPP = _po_bounds(rng, n), _po_bounds(rng, n)
    RR = _po_bounds(rng, n)
    RR[0] = RR[1]  # upper, upper, lower meet in case 0
    rf.RowModel().x3_step(RR, PPP, Q)
    with pytest.raises(rf.RowBoundError, match="Q - X3 leaves int32"):
        rf.RowModel(norm_x3=False).x3_step(RR, PPP, Q)
    mut = rf.RowModel(norm_x3=False)
    A = [rc.uniform_wave(rc.random_family(rng, t, 10000)) for t in rc.ROW_POINT]
    B = [rc.uniform_wave(rc.random_family(rng, t, 10000)) for t in rc.ROW_POINT]
    mut.xyzz_add_rows(A, B, rc.uniform_wave(rc.random_family(rng, "PO", 10000)))
    g = [rc.uniform_wave(rc.random_family(rng, t, 10000)) for t in ("E", "EY", "E", "EY")]
    mut.mmadd_pairs(*g)
    assert mut.stats["stored"] < 1 << 31


def test_w_as_p_plus_2u1_is_the_same_limbs():
    """rows.h once said the fused check sums U1 + U2 + r ZZ12 "instead of" P +
    2 U1 + r ZZ12 so that limbs fit int32.  The two are the same limbs: P = U2 -
    U1 limb by limb, so P + 2 U1 = U1 + U2 in every limb, in integers and (mod
    2^32) in the registers, whatever the order of the additions -- and every
    partial sum is bounded by the final one, < 3 2^29 + 2^6.  A model that
    forms w the other way therefore cannot trip an int32 assertion on any
    input; this test pins that equivalence (same verdicts, same w maximum, no
    bound error) on the bound families and on 10,000 random cases, and rows.h
    now says so."""
    rng = np.random.default_rng(6)
    for n, gen in ((512, rc.family), (10000, rc.random_family)):
        A = [rc.uniform_wave(gen(rng, t, n)) for t in rc.ROW_POINT]
        B = [rc.uniform_wave(gen(rng, t, n)) for t in rc.ROW_POINT]
        A[0][:4], B[0][:4] = rc.uniform_wave(rc.bound_family(rng, "PO", 22)[:4]), A[0][:4]
        rz = rc.uniform_wave(gen(rng, "PO", n))
        m1, m2 = rf.RowModel(), rf.RowModel(w_sum=False)
        r1, r2 = m1.xyzz_add_check_rows(A, B, rz), m2.xyzz_add_check_rows(A, B, rz)
        assert (r1[0] == r2[0]).all() and (r1[1] == r2[1]).all()
        assert m1.stats["w_max"] == m2.stats["w_max"] < rf.W_BOUND


# ---- the quad schedule composed from the harness ---------------------------------------
def _u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def _s32(x):
    return np.asarray(x, np.uint32).astype(np.int32).astype(np.int64)


def test_quad_restatement_values(H):  # noqa: F811
    """QuadModel (the harness's fs_mul / fs_norm in the device code's order)
    computes mmadd-2008-s, add-2008-s and the fused check's verdict"""
    q = rf.QuadModel(H)
    rng = np.random.default_rng(8)
    n = 512
    g = [rc.family(rng, t, n)[rng.permutation(n)] for t in ("S", "D", "S", "D")]
    rm = rc.family(rng, "FA", n)
    out, rz = q.mmadd(*[_u32(v) for v in g], _u32(rm))
    gp, o, rmp = [_plain(v) for v in g], [_plain(_s32(v)) for v in out], _plain(rm)
    rzp = _plain(_s32(rz))
    for i in range(n):
        want = rc.mmadd_formula(*[v[i] for v in gp])
        assert [v[i] for v in o] == want and rzp[i] == rmp[i] * want[2] % P
    A, B, rm, lab = rc.add_cases(rng, n, rc.QUAD_POINT, "FA", n_curve=128)
    qinf = rng.integers(0, 2, n).astype(bool)
    out, rz = q.add([_u32(A[:, k]) for k in range(4)], [_u32(B[:, k]) for k in range(4)], _u32(rm), qinf)
    Ap, Bp = [_plain(A[:, k]) for k in range(4)], [_plain(B[:, k]) for k in range(4)]
    o, rzp, rmp = [_plain(_s32(v)) for v in out], _plain(_s32(rz)), _plain(rm)
    for i in range(n):
        want, _ = rc.add_formula([a[i] for a in Ap], [b[i] for b in Bp])
        assert [v[i] for v in o] == want, lab[i]
        assert rzp[i] == rmp[i] * (Ap[2][i] if qinf[i] else want[2]) % P
    A, B, rz, want = rc.check_cases(rng, n, rc.QUAD_POINT, "S")
    ok, exc = q.add_check([_u32(A[:, k]) for k in range(4)], [_u32(B[:, k]) for k in range(4)], _u32(rz))
    Ap, Bp, rzp = [_plain(A[:, k]) for k in range(4)], [_plain(B[:, k]) for k in range(4)], _plain(rz)
    for i in range(n):
        w = rc.check_formula([a[i] for a in Ap], [b[i] for b in Bp], rzp[i])
        assert (bool(ok[i]), bool(exc[i])) == w, i
        assert w[1] == want[i][1] and (w[1] or w[0] == want[i][0]), i


def test_cpu_build_of_the_headers_equals_integers(H):  # noqa: F811
    """tests/cpp/field_ops.h through g++ (hb_NAME of libalgo_harness.so): every
    operation the GPU test compares limb for limb with the device build, on the
    same families at an eighth of the size, against Python integers -- the
    aliased calls (an output that is an operand) among the outputs"""
    import fieldops_cases as fc
    for j, name in enumerate(fc.C_OPS):
        ops, ex, inp = fc.c_inputs(name, np.random.default_rng(0xC000 + j), 1024)
        fc.check_values(name, ops, ex, fc.run_op(H, "hb_", name, inp))
