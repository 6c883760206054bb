"""The verify under unregistered keys on the CPU: simple_pbft_amd/csrc/varbase.h
(the limb code k_varbase runs) compiled with g++ (tests/cpp/varbase_harness.cpp)
and checked bit for bit against the oracle -- the golden vectors with the key
taken from the fixture, conftest.crafted_exceptional(), the crafted ladder /
G-part / key cases of tests/varbase_cases.py, and 2,000 oracle-signed random
signatures with 2 % corrupted.  The same harness, built as a stand-alone
program with the address and undefined-behaviour sanitizers, is run once."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import varbase_cases as vc
from conftest import ROOT, signed_digits

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "varbase_harness.cpp")
_CSRC = os.path.join(ROOT, "simple_pbft_amd", "csrc")
_HDRS = [os.path.join(_CSRC, f) for f in ("varbase.h", "p256_algo.h", "fe29.h", "fes.h", "safegcd.h", "p256_consts.h")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [_SRC])


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libvarbase_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.h_vb_g_table_words.restype = ctypes.c_uint64
    lib.h_vb_build_g_table.argtypes = [vp]
    lib.h_vb_digits.argtypes = [vp, vp]
    lib.h_vb_gdigits.argtypes = [vp, vp, vp]
    lib.h_vb_verify_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def gtab(H):
    """the width-16 comb table of G (34 MiB), built once by p256_algo.h's serial builder"""
    t = np.zeros(H.h_vb_g_table_words(), np.uint32)
    H.h_vb_build_g_table(t.ctypes.data)
    return t


def run(H, gtab, hashes, sigs, pubs):
    hashes, sigs, pubs = (np.ascontiguousarray(a, np.uint8) for a in (hashes, sigs, pubs))
    n = len(hashes)
    out, paths = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    H.h_vb_verify_batch(n, hashes.ctypes.data, sigs.ctypes.data, pubs.ctypes.data, gtab.ctypes.data, out.ctypes.data,
                        paths.ctypes.data)
    return out.astype(bool), paths


def words(u):
    return np.array([(u >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)


def test_recoding_matches_signed_digit_rule(H):
    """vb_recode's one addition gives the digits of signed_digit_w's rule at
    4 bits (conftest.signed_digits), in [-7, 8], summing back to u; the G
    part's shifted cut gives signed_digit_w<16>'s digits."""
    rng = np.random.default_rng(11)
    us = [0, 1, 7, 8, 9, 15, 16, 17, 1 << 128, vc.N - 1, vc.N - 2, int("8" * 64, 16), int("9" * 64, 16),
          int("7" * 64, 16), (1 << 256) - 1, int("f" * 63 + "8", 16)]
    us += [int.from_bytes(rng.bytes(32), "big") for _ in range(300)]
    for u in us:
        w = words(u)
        d = np.zeros(65, np.int32)
        H.h_vb_digits(w.ctypes.data, d.ctypes.data)
        assert d.tolist() == [x for x, _ in signed_digits(u, [4] * 65)], hex(u)
        assert all(-7 <= x <= 8 for x in d.tolist()) and d[64] in (0, 1)
        assert sum(int(x) << (4 * i) for i, x in enumerate(d.tolist())) == u
        g, ref = np.zeros(17, np.int32), np.zeros(17, np.int32)
        H.h_vb_gdigits(w.ctypes.data, g.ctypes.data, ref.ctypes.data)
        assert g.tolist() == ref.tolist() == [x for x, _ in signed_digits(u, [16] * 17)], hex(u)


def test_golden_vectors_with_their_keys(H, gtab, oracle_lib):
    h, s, p, want = vc.golden_set(oracle_lib)
    assert len(h) == 163
    got, _ = run(H, gtab, h, s, p)
    assert (got == want).all(), np.nonzero(got != want)[0]


def test_crafted_exceptional(H, gtab, oracle_lib):
    h, s, p, want = vc.exceptional_set(oracle_lib)
    got, paths = run(H, gtab, h, s, p)
    assert (got == want).all(), np.nonzero(got != want)[0]
    assert paths.any()  # equal scalars under Q = G meet in the G part


def test_crafted_ladder_gpart_and_keys(H, gtab, oracle_lib):
    h, s, p, want, names, rerun = vc.crafted_set(oracle_lib)
    got, paths = run(H, gtab, h, s, p)
    bad = [names[i] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    # the exact rerun runs where a meeting was built in, and nowhere in the plain ladder cases
    wrong = [names[i] for i, rr in enumerate(rerun) if rr is not None and bool(paths[i] & 1) != rr]
    assert not wrong, wrong
    assert want.any() and not want.all()


def test_random_signed_with_corruptions(H, gtab, oracle_lib):
    keys, h, s, kidx, p, bad = vc.random_signed(oracle_lib, 20, 100, seed=77, corrupt=0.02)
    assert len(h) == 2000 and bad.sum() == 40
    want = vc.oracle_expect(oracle_lib, h, s, p)
    assert want[~bad].all() and not want[bad].any()
    got, paths = run(H, gtab, h, s, p)
    assert (got == want).all(), np.nonzero(got != want)[0]
    assert not paths.any()  # honest scalars never meet


def test_stand_alone_program_under_sanitizers():
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only): the fast form and the exact rerun against the G comb
    alone on edge scalars and a random stream; any sanitizer report aborts it."""
    exe = os.path.join(_CPP, "varbase_san")
    if _stale(exe):
        # (shift-base off: fe29.h's carry folds shift negative limbs left on
        # purpose -- two's complement, what the GPU does and C++20 defines)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                        "-fno-sanitize-recover=all", "-DVARBASE_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe, "16"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "varbase: 0 mismatches" in p.stdout
