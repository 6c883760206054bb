"""sign.h on the device, one lane per case (tests/cpp/sign_probe.hip ->
libsign_probe.so): the RFC 6979 DRBG's first three candidates and
ecdsa_sign_with_k under chosen nonces, every word compared with
tests/rfc6979_model.py over the case lists of tests/sign_cases.py -- the lists
the CPU harness runs (tests/test_sign_cpu.py).  The library exports no
sign-with-k, so this is where the comb walk's digit seams reach hipcc's code."""
from __future__ import annotations

import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import sign_cases as sc
from conftest import ROOT
from test_sign_cpu import H, gtab  # noqa: F401  (libsign_harness.so and its G table, rebuilt when stale)

pytestmark = pytest.mark.gpu

HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics"]  # the library's


@pytest.fixture(scope="module")
def probe(gtab):  # noqa: F811
    d = os.path.join(ROOT, "tests", "cpp")
    so, src = os.path.join(d, "libsign_probe.so"), os.path.join(d, "sign_probe.hip")
    deps = [src] + glob.glob(os.path.join(ROOT, "simple_pbft_amd", "csrc", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as __graft_entry__.build() and the Makefile
        if not shutil.which(hipcc):
            pytest.fail("tests/cpp/libsign_probe.so is missing or older than its sources and there is no hipcc "
                        "to build it: run __graft_entry__.build()")
        subprocess.run([hipcc] + HIPFLAGS + ["-shared", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.sp_g_table_bytes.restype = ctypes.c_uint64
    lib.sp_set_g_table.argtypes = [vp]
    lib.sp_drbg.argtypes = [vp, vp, vp, ctypes.c_int]
    lib.sp_sign_with_k.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int]
    assert lib.sp_g_table_bytes() == gtab.nbytes
    assert lib.sp_set_g_table(gtab.ctypes.data) == 0
    yield lib
    lib.sp_release()


def test_drbg_first_three_candidates_on_the_device(probe):
    cases = sc.drbg_cases()
    want = sc.drbg_expected(cases, 3)
    d, h = sc.col([c[0] for c in cases]), sc.col([c[1] for c in cases])
    got = np.zeros_like(want)
    assert probe.sp_drbg(d.ctypes.data, h.ctypes.data, got.ctypes.data, len(cases)) == 0
    assert (got == want).all(), np.nonzero((got != want).any(axis=(1, 2)))[0]


def test_sign_with_chosen_k_on_the_device(probe):
    """Range ends, single windows, the recoding-carry seam (0x8000 / 0x8001 /
    0x7FFF alone and in runs to the top window) and all ones, crossed with the
    ends of e and d: (r, s) equal to the model's, ok everywhere, no rerun."""
    cases = sc.with_k_cases()
    want_rs, want_ok = sc.with_k_expected()
    e, d, k = (sc.col([c[j] for c in cases]) for j in range(3))
    n = len(cases)
    rs, ok, path = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint32), np.full(n, 9, np.uint32)
    assert probe.sp_sign_with_k(e.ctypes.data, d.ctypes.data, k.ctypes.data, rs.ctypes.data, ok.ctypes.data,
                                path.ctypes.data, n) == 0
    assert (ok.astype(bool) == want_ok).all() and want_ok.all()
    assert (rs == want_rs).all(), np.nonzero((rs != want_rs).any(axis=1))[0]
    assert not path.any()


def test_sign_with_k_out_of_range_on_the_device(probe):
    ks = [0, sc.N, sc.N + 1, sc.TOP]
    n = len(ks)
    e, d, k = sc.col([5] * n), sc.col([7] * n), sc.col(ks)
    rs, ok, path = np.full((n, 64), 0xEE, np.uint8), np.ones(n, np.uint32), np.zeros(n, np.uint32)
    assert probe.sp_sign_with_k(e.ctypes.data, d.ctypes.data, k.ctypes.data, rs.ctypes.data, ok.ctypes.data,
                                path.ctypes.data, n) == 0
    assert not ok.any() and not rs.any()
