"""The signed-limb products' two schedules (simple_pbft_amd/csrc/fes.h): the
column-order upper half that the kernels run (fs_mul, fs_sqr, fs_sqr_sub2,
fs_mul2_add, fs_sqr_mul_add) against the kept row schedule (*_rows), limb for
limb, and against Python integers.  Compiled for the CPU
(tests/cpp/fs_columns_harness.cpp); the same harness, built as a stand-alone
program with the address and undefined-behaviour sanitizers, is run once."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
R = 1 << 261
RINV = pow(R, -1, P)
M29 = (1 << 29) - 1
S_BOUND = int(2 ** 257.5)
OPS = {"mul": 0, "sqr": 1, "sqr_sub2": 2, "mul2_add": 3, "sqr_mul_add": 4}
# operand types the header allows, per op: "x" = S or D, "S" = S only, "-" = unused
TYPES = {"mul": "xx--", "sqr": "x---", "sqr_sub2": "xSS-", "mul2_add": "xxxx", "sqr_mul_add": "xSS-"}

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "fs_columns_harness.cpp")
_HDRS = [os.path.join(ROOT, "simple_pbft_amd", "csrc", f) for f in ("fe29.h", "fes.h", "p256_consts.h")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [_SRC])


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libfs_columns_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.h_fsc_batch.restype = ctypes.c_uint64
    lib.h_fsc_batch.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def run(H, op, sets):
    """sets: (n, 4, 9) signed limbs -> (n, 9) uint32 limbs of the column-order
    product, after asserting that the row schedule gives the same limbs"""
    inp = np.ascontiguousarray(np.asarray(sets, np.int64).astype(np.uint32).reshape(-1, 36))
    n = len(inp)
    cols, rows = np.zeros((n, 9), np.uint32), np.zeros((n, 9), np.uint32)
    bad = H.h_fsc_batch(OPS[op], n, inp.ctypes.data, cols.ctypes.data, rows.ctypes.data)
    diff = np.nonzero((cols != rows).any(axis=1))[0]
    assert bad == 0 and len(diff) == 0, (op, diff[:5], inp[diff[:1]])
    return cols


def sval(l):
    return sum(int(np.int32(np.uint32(x))) << (29 * i) for i, x in enumerate(l))


def lval(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def s_limbs_of(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def expect_T(op, a, b, c, d):
    """the integer whose Montgomery reduction the op returns"""
    return {"mul": a * b, "sqr": a * a, "sqr_sub2": a * a - (b + 2 * c) * R, "mul2_add": a * b + c * d,
            "sqr_mul_add": a * a + b * c}[op]


def check_values(op, sets, out, typed=True):
    for s, o in zip(sets, out):
        a, b, c, d = (lval(x) for x in s)
        v = sval(o)
        assert v * R % P == expect_T(op, a, b, c, d) % P, (op, s)
        if typed:
            assert all(0 <= int(x) < (1 << 29) for x in o[:8]), (op, s)
            if op in ("mul", "sqr", "sqr_mul_add"):  # one product (or the fused step's pair): |T| / R + 1.0001 p
                assert abs(v) < S_BOUND, (op, s)


def rand_s_np(rng, n):
    """n S-type values: limbs 0..7 in [0, 2^29), limb 8 signed, |value| < 2^257.5"""
    l = rng.integers(0, 1 << 29, (n, 9), dtype=np.int64)
    top = int(S_BOUND >> 232) - 1
    l[:, 8] = rng.integers(-top, top + 1, n)
    return l


def rand_sets(rng, op, n):
    """n operand sets of every type pairing the op allows (S or D per operand,
    by the bits of the set's index)"""
    sets = np.zeros((n, 4, 9), np.int64)
    for k, t in enumerate(TYPES[op]):
        if t == "-":
            continue
        s = rand_s_np(rng, n)
        if t == "x":
            is_d = (np.arange(n) >> k) & 1 == 1
            s = s - rand_s_np(rng, n) * is_d[:, None]
        sets[:, k] = s
    return sets


@pytest.mark.parametrize("op", list(OPS))
def test_random_inputs_limb_identity_and_values(H, op):
    rng = np.random.default_rng(0xC015 + OPS[op])
    sets = rand_sets(rng, op, 40000)
    out = run(H, op, sets)
    check_values(op, sets[:1500].tolist(), out[:1500])


def _bound_sets(op):
    """inputs at the bounds, as (sets, typed): typed ones lie inside the
    documented S / D types, the others only inside the limb bounds"""
    top = [M29] * 9
    typed, raw = [], []
    used = [k for k, t in enumerate(TYPES[op]) if t != "-"]
    # every limb at +-(2^29 - 1): all sign pairings, whole operands and
    # alternating limbs.  An S-only operand (fs_sqr_sub2's b and c, whose limbs
    # enter the columns as b_k + 2 c_k, and fs_sqr_mul_add's) keeps the shape of
    # its type: limbs 0..7 at 2^29 - 1, limb 8 at the type's signed extreme.
    s8 = int(S_BOUND >> 232) - 1
    for signs in range(1 << len(used)):
        for alt in (False, True):
            s = [[0] * 9 for _ in range(4)]
            for n, k in enumerate(used):
                if TYPES[op][k] == "S":
                    s[k] = [M29] * 8 + [-s8 if (signs >> n) & 1 else s8]
                else:
                    s[k] = [(-x if ((signs >> n) ^ (i if alt else 0)) & 1 else x) for i, x in enumerate(top)]
            raw.append(s)
    raw.append([[0] * 9 for _ in range(4)])
    typed.append([[0] * 9 for _ in range(4)])
    # limb 8 at its signed extremes: S-type values next to +-2^257.5 with low
    # limbs all-ones or zero, and D-type differences of two such
    ext = []
    for sign in (1, -1):
        for low in (0, M29):
            l = s_limbs_of(sign * (S_BOUND - 1))
            l[:8] = [low] * 8
            while abs(lval(l)) >= S_BOUND:
                l[8] -= sign
            ext.append(l)
    d_ext = [[x - y for x, y in zip(a, b)] for a in ext for b in ext if a is not b]
    for i in range(24):
        s = [[0] * 9 for _ in range(4)]
        for n, k in enumerate(used):
            pool = ext if TYPES[op][k] == "S" or (i >> n) & 1 == 0 else d_ext
            s[k] = pool[(i * 5 + 3 * n) % len(pool)]
        typed.append(s)
    # the multiples k p, |k| <= 5: every one of the eleven in each operand that
    # takes a D-type value, and those an S-type value can hold in each operand
    rng = np.random.default_rng(0xC0FE)
    kp_s, kp_d = kp_forms(rng)
    other = rand_s_np(rng, 16).tolist()
    for pos in used:
        forms = list(kp_s.items()) + (list(kp_d.items()) if TYPES[op][pos] == "x" else [])
        for i, (k, m) in enumerate(forms):
            s = [other[(i + 1 + j) % len(other)] if j in used else [0] * 9 for j in range(4)]
            s[pos] = m
            typed.append(s)
    return typed, raw


def kp_forms(rng):
    """The multiples k p, |k| <= 5, as {k: limbs}: S-type where the type holds
    the value (|k p| < 2^257.5: |k| <= 2), and D-type for all eleven, as the
    limb-wise difference of two S-type values next to k p / 2 and -k p / 2
    (|k p / 2| <= 2^257.33, so an offset below 2^254 keeps both inside the type)."""
    kp_s = {k: s_limbs_of(k * P) for k in range(-5, 6) if abs(k * P) < S_BOUND}
    kp_d = {}
    for k in range(-5, 6):
        off = int(rng.integers(-(1 << 62), 1 << 62)) << 191
        x = k * P // 2 + off
        y = x - k * P
        assert abs(x) < S_BOUND and abs(y) < S_BOUND
        kp_d[k] = [u - v for u, v in zip(s_limbs_of(x), s_limbs_of(y))]
    return kp_s, kp_d


def test_every_multiple_of_p_is_among_the_bound_inputs():
    """All eleven k p reach every operand that takes a D-type value (and k p,
    |k| <= 2, every operand, as S-type values): none is dropped by a draw."""
    kp_s, kp_d = kp_forms(np.random.default_rng(0xC0FE))
    assert sorted(kp_s) == list(range(-2, 3)) and sorted(kp_d) == list(range(-5, 6))
    for k in range(-5, 6):
        assert lval(kp_d[k]) == k * P and all(abs(x) < (1 << 29) for x in kp_d[k][:8])
        if k in kp_s:
            assert lval(kp_s[k]) == k * P and all(0 <= x < (1 << 29) for x in kp_s[k][:8])
    for op in OPS:
        typed, _ = _bound_sets(op)
        for pos, t in enumerate(TYPES[op]):
            if t == "-":
                continue
            seen_s = {k for k in kp_s if any(s[pos] == kp_s[k] for s in typed)}
            seen_d = {k for k in kp_d if any(s[pos] == kp_d[k] for s in typed)}
            assert seen_s == set(kp_s), (op, pos)
            if t == "x":
                assert seen_d == set(kp_d), (op, pos)


@pytest.mark.parametrize("op", list(OPS))
def test_inputs_at_the_bounds(H, op):
    typed, raw = _bound_sets(op)
    check_values(op, typed, run(H, op, typed), typed=True)
    check_values(op, raw, run(H, op, raw), typed=False)


def test_all_maximum_column_magnitude():
    """The all-maximum fs_mul2_add input is the documented worst column: 18
    products of (2^29 - 1)^2 in column 8 (2^62.17) plus the digit terms of
    columns 0..5 and 1, 2 (each digit < 2^32, constants 2^9, 2^18, 2^29 - 2^21,
    2^24 - 1: < 2^61.1), inside int64 -- the case test_inputs_at_the_bounds
    runs through both schedules."""
    col = 18 * M29 * M29
    digits = (1 << 32) * ((1 << 9) + (1 << 18) + (1 << 29) - (1 << 21) + (1 << 24) - 1)
    assert 2 ** 62.1 < col < 2 ** 62.2 and digits < 2 ** 61.1 and col + digits < 2 ** 63


def test_product_over_its_own_operand(H):
    """fs_mul(r, r, b): the output limbs are stored after the last column has
    read the operands"""
    rng = np.random.default_rng(0xA11A5)
    sets = rand_sets(rng, "mul", 200)
    want = run(H, "mul", sets)
    out = (ctypes.c_uint32 * 9)()
    for s, w in zip(sets, want):
        a = (ctypes.c_uint32 * 9)(*[int(x) & 0xFFFFFFFF for x in s[0]])
        b = (ctypes.c_uint32 * 9)(*[int(x) & 0xFFFFFFFF for x in s[1]])
        H.h_fsc_mul_inplace(a, b, out)
        assert list(out) == w.tolist()


def test_sqr_sub2_over_its_subtrahends(H):
    """fs_sqr_sub2 with r over b or c, in both schedules, and fs_sqr_sub2_mul
    with r2 over b or c: limb 8 of b and c is read before any result is stored"""
    rng = np.random.default_rng(0xA11A6)
    sets = rand_sets(rng, "sqr_sub2", 200)
    want = run(H, "sqr_sub2", sets)
    e, f = rand_s_np(rng, 200), rand_s_np(rng, 200)
    mul = np.zeros((200, 4, 9), np.int64)
    mul[:, 0], mul[:, 1] = e, f
    want_ef = run(H, "mul", mul)
    out = (ctypes.c_uint32 * 36)()
    for i in range(200):
        five = np.concatenate([sets[i, :3].reshape(-1), e[i], f[i]]).astype(np.uint32)
        for over in (1, 2):
            H.h_fsc_sqr_sub2_over(over, five.ctypes.data_as(ctypes.c_void_p), out)
            got = np.array(out, np.uint32).reshape(4, 9)
            assert (got[:3] == want[i]).all() and (got[3] == want_ef[i]).all(), (i, over)


def test_paired_addition_limb_identity(H):
    """A chain of 300 comb additions (S-type accumulator, canonical entries with
    random y signs) on the row-schedule products, on lone column chains and on
    the paired form the comb runs (fs_reduce2: U2 | S2, PPP | Q, X3 | ZZ3,
    Y3 | ZZZ3): the same limbs after every step."""
    rng = np.random.default_rng(0xADD5)
    start = rand_s_np(rng, 4).astype(np.uint32).reshape(-1)
    accs = [(ctypes.c_uint32 * 36)(*start.tolist()) for _ in range(3)]
    for step in range(300):
        x, y = (int.from_bytes(rng.bytes(32), "big") % P for _ in range(2))
        ly = [(x_ >> (29 * i)) & M29 for i in range(9) for x_ in [y]]
        if rng.integers(0, 2):
            ly = [(-v) & 0xFFFFFFFF for v in ly]
        pt = (ctypes.c_uint32 * 18)(*[(x >> (29 * i)) & M29 for i in range(9)], *ly)
        for variant, acc in enumerate(accs):
            H.h_fsc_madd(variant, acc, pt)
        assert list(accs[0]) == list(accs[1]) == list(accs[2]), step


def test_stand_alone_program_under_sanitizers():
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only), compares the two schedules on the bound inputs and a
    random stream; any sanitizer report aborts it."""
    exe = os.path.join(_CPP, "fs_columns_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DFS_COLUMNS_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "fs_columns: 0 mismatches" in p.stdout
