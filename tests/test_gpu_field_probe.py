"""The latency path's field arithmetic on the device, one operation at a time
(tests/cpp/field_probe.hip -> libfield_probe.so), against exact integers:

  A. rows.h -- every one of a wave's 64 output lanes equals tests/rowfield.py's
     limb-exact model (so lanes 9..15 are 0 and the rows do not disturb each
     other: a wave's four rows carry four different cases);
  B. the quad schedule and fmont_lane of verify_kernels.h -- limbs equal the
     CPU harness's products composed in the device code's order, in every lane
     of the quad; fmont_lane by value, range and limb width;
  C. fes.h / fe29.h / p256_algo.h / sec1.h as hipcc compiles them for gfx950
     (inline-asm opaque limbs, builtin bit ops, the compiler's choice of
     multiply-add forms) -- limbs equal the g++ build's (libalgo_harness.so,
     the same wrappers of tests/cpp/field_ops.h), and both equal Python
     integers mod p (mod n for fn_mul).

The inputs are the families of tests/rowfield_cases.py: every limb at its type
bound, the special values in every type, random ones, curve points, doublings
and cancellations, 4-level chains, and the fused check's accept / reject / exc
cases.  Expectations are built once per module.
"""
from __future__ import annotations

import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import rowfield as rf
import rowfield_cases as rc
from rowfield_suite import row_suite
from conftest import ROOT
from fieldops_cases import C_OPS, c_inputs, check_values, run as _run, run_op, u32 as _u32
from rowfield_cases import N, P
from test_algo_cpu import H  # noqa: F401  (libalgo_harness.so, rebuilt when stale)

pytestmark = pytest.mark.gpu

N_WAVES = 4096  # A, B: cases per operation (one wave or quad each)
N_LANES = 8192  # C: cases per operation (one lane each)
HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics"]  # the library's


@pytest.fixture(scope="module")
def probe():
    d = os.path.join(ROOT, "tests", "cpp")
    so, src = os.path.join(d, "libfield_probe.so"), os.path.join(d, "field_probe.hip")
    deps = [src, os.path.join(d, "field_ops.h")] + glob.glob(os.path.join(ROOT, "simple_pbft_amd", "csrc", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as __graft_entry__.build() and the Makefile
        if not shutil.which(hipcc):
            pytest.fail("tests/cpp/libfield_probe.so is missing or older than its sources and there is no hipcc "
                        "to build it: run __graft_entry__.build()")
        subprocess.run([hipcc] + HIPFLAGS + ["-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


def _wave(*vals):
    """row values (n, 4, 16) -> the probe's input (n, K * 64)"""
    return np.concatenate([_u32(v).reshape(len(v), 64) for v in vals], axis=1)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not (got == want).all():
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: got 0x%08x, want 0x%08x"
                             % (what, len(bad), got.size, i, int(got[i]), int(want[i])))


# ---- A. rows ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def suite():
    return row_suite(N_WAVES)


def test_row_mul(probe, suite):
    c = suite["row_mul"]
    _same(_run(probe, "fp_row_mul", _wave(c["a"], c["b"]), 64), _wave(c["out"]), "row_mul")


def test_row_norm(probe, suite):
    c = suite["row_norm"]
    _same(_run(probe, "fp_row_norm", _wave(c["x"]), 64), _wave(c["out"]), "row_norm")


def test_gather4_sel4(probe):
    """every row sees g[0..3]; row r takes v_r -- on arbitrary register contents"""
    rng = np.random.default_rng(41)
    x = rng.integers(0, 1 << 32, (N_WAVES, 5, 4, 16), dtype=np.uint64).astype(np.uint32)
    x[:64, :, :, :] &= np.uint32(0xF)  # (near-equal rows: a swap of two would still show)
    x[:64, 0] += (np.arange(4, dtype=np.uint32) << 8)[None, :, None]
    got = _run(probe, "fp_gather_sel", x.reshape(N_WAVES, 320), 320).reshape(N_WAVES, 5, 4, 16)
    for r in range(4):
        _same(got[:, r], np.broadcast_to(x[:, 0, r:r + 1], (N_WAVES, 4, 16)), "gather4 g[%d]" % r)
    _same(got[:, 4], np.stack([x[:, 1 + r, r] for r in range(4)], axis=1), "sel4")


def _add_in(A, B, rm):
    w = rc.uniform_wave
    return _wave(*[w(A[:, k]) for k in range(4)], *[w(B[:, k]) for k in range(4)], w(rm))


def test_xyzz_add_rows(probe, suite):
    c = suite["add"]
    got = _run(probe, "fp_xyzz_add_rows", _add_in(c["A"], c["B"], c["rm"]), 320)
    _same(got, _wave(*c["out"], c["rz"]), "xyzz_add_rows")


def test_xyzz_add_rows_chain(probe, suite):
    """iv: four levels, outputs feeding inputs (a doubling or cancellation at
    level 1 keeps ZZ == 0 to the top: tests/test_rowfield.py checks the values)"""
    for lv, L in enumerate(suite["chain"]["levels"]):
        got = _run(probe, "fp_xyzz_add_rows", _wave(*L["A"], *L["B"], L["rm"]), 320)
        _same(got, _wave(*L["out"], L["rz"]), "level %d" % (lv + 1))


def test_mmadd_pairs(probe, suite):
    c = suite["mmadd"]
    _same(_run(probe, "fp_mmadd_pairs", _wave(*c["ins"]), 256), _wave(*c["out"]), "mmadd_pairs")


def test_xyzz_add_check_rows(probe, suite):
    """the verdict (ballot bit 0) and exc (bit 32), the same in all 64 lanes"""
    c = suite["check"]
    got = _run(probe, "fp_xyzz_add_check_rows", _add_in(c["A"], c["B"], c["rz"]), 128).reshape(-1, 2, 64)
    assert c["ok"].any() and c["exc"].any() and (~c["ok"] & ~c["exc"]).any()
    _same(got[:, 0], np.repeat(c["ok"][:, None], 64, 1), "verdict")
    _same(got[:, 1], np.repeat(c["exc"][:, None], 64, 1), "exc")


def test_row_is_zero_and_row_to_fe(probe, suite):
    c = suite["zero"]
    got = _run(probe, "fp_row_zero_fe", _wave(c["x"]), 640).reshape(-1, 10, 64)
    _same(got[:, 0], np.repeat(c["out"][:, None], 64, 1), "row_is_zero")
    _same(got[:, 1:], np.repeat(_u32(c["x"][:, 0, :9])[:, :, None], 64, 2), "row_to_fe")


def test_row_entry(probe):
    """vi: 0, 1, p - 1, 2^256 - 1 and single bits at every limb seam; both digit signs"""
    tab = rc.entry_table()
    ents = len(tab)
    digs = np.array([d for d in range(-ents, ents + 1)] * 8, np.int32)
    digs = np.random.default_rng(43).permutation(digs)[:len(digs) // 4 * 4]
    n = len(digs) // 4
    out = np.zeros((n, 2, 4, 16), np.uint32)
    probe.fp_row_entry.restype = ctypes.c_int
    err = probe.fp_row_entry(ctypes.c_void_p(tab.ctypes.data), ents, ctypes.c_void_p(digs.ctypes.data),
                             ctypes.c_void_p(out.ctypes.data), n)
    assert err == 0, err
    want = np.array([[rf.row_entry(tab, int(d), L) for L in range(16)] for d in digs], np.uint32).reshape(n, 4, 16, 2)
    _same(out[:, 0], want[..., 0], "row_entry x")
    _same(out[:, 1], want[..., 1], "row_entry y")
    bad = np.array([ents + 1, 0, 0, 0], np.int32)  # a digit past the table is refused, not read
    assert probe.fp_row_entry(ctypes.c_void_p(tab.ctypes.data), ents, ctypes.c_void_p(bad.ctypes.data),
                              ctypes.c_void_p(out.ctypes.data), 1) == -1


# ---- B. quads, fmont_lane --------------------------------------------------------------
def _pt(A):
    return [_u32(A[:, k]) for k in range(4)]


def _quad_out(got, n):
    """(n, 4 lanes, 45): x, y, zz, zzz, rz per lane"""
    return got.reshape(n, 4, 5, 9)


def test_quad_mul(probe, H):  # noqa: F811
    rng = np.random.default_rng(51)
    n = N_WAVES
    ops = [rc.family(rng, ("S", "D")[(k // 2 + k) & 1], n) for k in range(8)]
    ops = [v if k < 2 else v[rng.permutation(n)] for k, v in enumerate(ops)]
    got = _run(probe, "fp_quad_mul", np.concatenate([_u32(v) for v in ops], axis=1), 36).reshape(n, 4, 9)
    q = rf.QuadModel(H)
    for role in range(4):
        _same(got[:, role], q.mul(_u32(ops[2 * role]), _u32(ops[2 * role + 1])), "role %d" % role)


def test_quad_mmadd_xyzz(probe, H):  # noqa: F811
    rng = np.random.default_rng(52)
    n = N_WAVES
    (gx, gy, qx, qy), _ = rc.mmadd_cases(rng, n)
    g = [_u32(v) for v in (gx, gy, qx, qy)]
    rm = _u32(rc.family(rng, "FA", n))
    got = _quad_out(_run(probe, "fp_quad_mmadd", np.concatenate(g + [rm], axis=1), 180), n)
    out, rz = rf.QuadModel(H).mmadd(*g, rm)
    for lane in range(4):
        for k, w in enumerate(out + [rz]):
            _same(got[:, lane, k], w, "lane %d, value %d" % (lane, k))


def test_quad_xyzz_add(probe, H):  # noqa: F811
    """with qinf false and true; curve points, doublings, cancellations, a zero ZZ"""
    rng = np.random.default_rng(53)
    n = N_WAVES
    A, B, rm, _ = rc.add_cases(rng, n, rc.QUAD_POINT, "FA")
    qinf = rng.integers(0, 2, n).astype(bool)
    inp = np.concatenate(_pt(A) + _pt(B) + [_u32(rm), qinf.astype(np.uint32)[:, None]], axis=1)
    got = _quad_out(_run(probe, "fp_quad_add", inp, 180), n)
    out, rz = rf.QuadModel(H).add(_pt(A), _pt(B), _u32(rm), qinf)
    for lane in range(4):
        for k, w in enumerate(out + [rz]):
            _same(got[:, lane, k], w, "lane %d, value %d" % (lane, k))


def test_quad_xyzz_add_check(probe, H):  # noqa: F811
    rng = np.random.default_rng(54)
    n = N_WAVES
    A, B, rz, want = rc.check_cases(rng, n // 2, rc.QUAD_POINT, "S")
    A2, B2, rz2, _ = rc.add_cases(rng, n // 2, rc.QUAD_POINT, "S", n_curve=0)
    A, B, rz = np.concatenate([A, A2]), np.concatenate([B, B2]), np.concatenate([rz, rz2])
    got = _run(probe, "fp_quad_add_check", np.concatenate(_pt(A) + _pt(B) + [_u32(rz)], axis=1), 8).reshape(n, 4, 2)
    ok, exc = rf.QuadModel(H).add_check(_pt(A), _pt(B), _u32(rz))
    for i, (w_ok, w_exc) in enumerate(want):  # the crafted cases come out as crafted
        assert bool(exc[i]) == w_exc and (w_exc or bool(ok[i]) == w_ok), i
    assert ok.any() and exc.any() and (~ok & ~exc).any()
    for lane in range(4):
        _same(got[:, lane, 0], ok, "verdict, lane %d" % lane)
        _same(got[:, lane, 1], exc, "exc, lane %d" % lane)


def test_fmont_lane(probe):
    """vii: a to 2^257 - 1, b to 2^261 - 1; 0, 1, n - 1, n, p - 1, p; lanes 0, 1
    of a quad mod n, lanes 2, 3 mod p: the value mod the lane's modulus, the
    output < a b / 2^261 + m, limbs < 2^29"""
    rng = np.random.default_rng(55)
    n = N_WAVES
    a, b = rc.bound_family(rng, "FA", n), rc.bound_family(rng, "FB", n)
    sp = [0, 1, N - 1, N, P - 1, P]
    for j, (x, y) in enumerate((x, y) for x in sp for y in sp):  # every special pair, mod n (lane 0) and mod p (lane 2)
        a[64 + 4 * j], b[64 + 4 * j] = rc.s_limbs_of(x), rc.s_limbs_of(y)
        a[66 + 4 * j], b[66 + 4 * j] = rc.s_limbs_of(x), rc.s_limbs_of(y)
    a[4:8], b[4:8] = a[0], b[0]  # all limbs at the upper bound, in each of the quad's lanes
    a[n // 2:], b[n // 2:] = rc.random_family(rng, "FA", n - n // 2), rc.random_family(rng, "FB", n - n // 2)
    got = _run(probe, "fp_fmont_lane", np.concatenate([_u32(a), _u32(b)], axis=1), 9)
    assert int(got.max()) < 1 << 29
    for i, (x, y, v) in enumerate(zip(rc.values(a), rc.values(b), rc.values(got.astype(np.int64)))):
        m = N if i & 3 < 2 else P
        assert v % m == x * y * pow(rc.R, -1, m) % m, i
        assert v * rc.R < x * y + m * rc.R, i


def _words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _wval(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def test_wave_scalars_products(probe):
    """wave_scalars and wave_scalars_lds: the call sites that give fmont_lane
    its modulus and digit constant by lane (mod n with kNPrime, mod p with 1).
    u1 = e / s, u2 = r / s mod n, r R and (r + n) R mod p, r + n < p; r and s
    at 1, n - 1 and on both sides of p - n; e at 0, n, 2^256 - 1."""
    rng = np.random.default_rng(56)
    n = 1024
    edge_rs = [1, 2, N - 1, N - 2, P - N - 1, P - N, P - N + 1, 1 << 255, (1 << 128) - 1]
    edge_e = [0, 1, N - 1, N, N + 1, P, 2 ** 256 - 1]
    cases = [(e, r, s) for e in edge_e for r in edge_rs for s in (1, N - 1, 0x1234567)]
    cases += [(e, 1 + int.from_bytes(rng.bytes(32), "big") % (N - 1), s) for e in edge_e for s in edge_rs]
    while len(cases) < n:
        cases.append(tuple(int.from_bytes(rng.bytes(32), "big") % m for m in (1 << 256, N, N)))
    cases = [(e, r or 1, s or 1) for e, r, s in cases[:n]]
    inp = np.array([_words(e) + _words(r) + _words(s) for e, r, s in cases], np.uint32)
    got = _run(probe, "fp_wave_scalars", inp, 60)
    assert int(got[:, 16:34].max()) < 1 << 29 and int(got[:, 51:60].max()) < 1 << 29
    rm, rnm, rml = (rc.values(got[:, a:a + 9].astype(np.int64)) for a in (16, 25, 51))
    for i, (e, r, s) in enumerate(cases):
        w = pow(s, -1, N)
        assert _wval(got[i, 0:8]) == e * w % N and _wval(got[i, 8:16]) == r * w % N, i
        assert _wval(got[i, 35:43]) % N == e * w % N and _wval(got[i, 43:51]) % N == r * w % N, i
        assert rm[i] % P == r * rc.R % P and rm[i] < 2 * P and rml[i] == rm[i], i
        assert got[i, 34] == (r + N < P), i
        if r + N < P:  # (otherwise rnm is never read; past 2^256 the eight words of r + n wrap)
            assert rnm[i] % P == (r + N) * rc.R % P and rnm[i] < 2 * P, i
    assert 0 < int(got[:, 34].sum()) < n


# ---- C. the CPU-tested headers as the device compiles them -------------------------------
@pytest.fixture(scope="module")
def c_cases(H):  # noqa: F811
    """every C operation's inputs and the g++ build's outputs, checked against Python integers"""
    cases = {}
    for j, name in enumerate(C_OPS):
        rng = np.random.default_rng(0xC000 + j)
        ops, ex, inp = c_inputs(name, rng, N_LANES)
        out = run_op(H, "hb_", name, inp)
        check_values(name, ops, ex, out)
        cases[name] = (inp, out)
    return cases


@pytest.mark.parametrize("name", list(C_OPS))
def test_device_build_matches_cpu_build(probe, c_cases, name):
    inp, want = c_cases[name]
    _same(run_op(probe, "fp_", name, inp), want, name)
