"""The carried-key verify swept at its seams, on the CPU: the families of
tests/carried_cases.py (chosen-scalar signatures under keys nobody holds the
private scalar of: ladder digits, G-comb digits and meetings, keys with edge
coordinates, a sweep of compressed X) through the g++ builds of the device limb
code -- tests/cpp/varbase_harness.cpp (h_vb_verify_batch, which also returns
whether the exact rerun ran) and tests/cpp/sec1_harness.cpp (h_sec1_decode,
h_sec1_verify_batch) -- against the oracle's bits, the pinned rerun bits and
Python's big-integer decode.  A compressed key WITHOUT a point that the decode
wrongly accepted is directly visible only here (the GPU shows accept bits, and
such a key's signature is rejected under almost any point): h_sec1_decode's
verdict and coordinates are compared for every key of the sweep.  The two
harnesses' stand-alone programs, built with the address and undefined-behaviour
sanitizers, walk a dump of the combined set once."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import carried_cases as cc
import wirekey_cases as wc
from conftest import ROOT
from wirekey_cases import KEY_COMPRESSED, KEY_UNCOMPRESSED, KEY_XY

_CPP = os.path.join(ROOT, "tests", "cpp")
_CSRC = os.path.join(ROOT, "simple_pbft_amd", "csrc")
_HDRS = [os.path.join(_CSRC, f) for f in ("sec1.h", "varbase.h", "p256_algo.h", "fe29.h", "fes.h", "safegcd.h",
                                          "p256_consts.h")] + [os.path.join(_CPP, "carried_dump.h")]
_SAN = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
        "-fno-sanitize-recover=all"]  # (as test_varbase_cpu.py / test_sec1_cpu.py build them)


def _stale(out, src):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [src])


def _shared(name):
    src, so = os.path.join(_CPP, name + ".cpp"), os.path.join(_CPP, "lib%s.so" % name)
    if _stale(so, src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def VB():
    lib, vp = _shared("varbase_harness"), ctypes.c_void_p
    lib.h_vb_g_table_words.restype = ctypes.c_uint64
    lib.h_vb_build_g_table.argtypes = [vp]
    lib.h_vb_verify_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
    lib.h_vb_gdigits.argtypes = [vp, vp, vp]
    lib.h_vb_digits.argtypes = [vp, vp]
    return lib


@pytest.fixture(scope="module")
def S1():
    lib, vp = _shared("sec1_harness"), ctypes.c_void_p
    lib.h_sec1_decode.argtypes = [ctypes.c_uint64, vp, ctypes.c_int, vp, vp]
    lib.h_sec1_verify_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, ctypes.c_int, vp, vp]
    return lib


@pytest.fixture(scope="module")
def gtab(VB):
    t = np.zeros(VB.h_vb_g_table_words(), np.uint32)
    VB.h_vb_build_g_table(t.ctypes.data)
    return t


def vb_run(VB, gtab, h, s, xy):
    n = len(h)
    out, paths = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    VB.h_vb_verify_batch(n, h.ctypes.data, s.ctypes.data, xy.ctypes.data, gtab.ctypes.data, out.ctypes.data,
                         paths.ctypes.data)
    return out.astype(bool), (paths & 1).astype(bool)


def s1_run(S1, gtab, h, s, keys, fmt):
    out = np.zeros(len(h), np.uint8)
    S1.h_sec1_verify_batch(len(h), h.ctypes.data, s.ctypes.data, keys.ctypes.data, fmt, gtab.ctypes.data,
                           out.ctypes.data)
    return out.astype(bool)


def s1_decode(S1, keys, fmt):
    n = len(keys)
    xy, ok = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8)
    S1.h_sec1_decode(n, keys.ctypes.data, fmt, xy.ctypes.data, ok.ctypes.data)
    return xy, ok.astype(bool)


def named(names, mask):
    return [names[i] for i in np.nonzero(mask)[0]][:6]


def test_keys_and_construction(oracle_lib):
    """KEYS holds the edge points (x = 0, 2^32, p - 3; Montgomery-form x with
    all limbs full, a short top limb, one top bit, a low limb less one -- the
    scan offsets are asserted in carried_cases.keys()), and chosen_sig under a key without a
    known private scalar verifies in Python's own restatement too"""
    K = cc.keys()
    assert len(K) == 15 and sum(1 for k in K if k[2] is not None) == 5
    xs = {q[0] for _, q, _ in K}
    assert {0, 1 << 32, cc.P - 3} <= xs
    assert {(cc.P - 1), (1 << 232) - 1, 1 << 255, (1 << 29) - 2} <= {x * cc.R261 % cc.P for x in xs}
    q = K[-1][1]
    for variant, want in ((cc.PLAIN, True), (cc.FLIP_R, False)):
        h, rs, w = cc.chosen_sig(q, 12345, cc.N - 77, variant)
        assert w == want == cc.p256.verify(h, int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big"), *q)
    h, rs, w = cc.chosen_sig(q, 0, 99, cc.E_PLUS_N)
    assert w and h == cc.N.to_bytes(32, "big")


def test_digits_of_the_chosen_scalars(VB, oracle_lib):
    """vb_next_gdigit and vb_recode cut every chosen scalar into the digits the
    cases were built for (conftest.signed_digits).  The accept bit cannot pin
    the comb's carry rule: 32768 recoded as -32768 with a carry is another
    valid recoding of the same scalar and sums to the same point."""
    def words(u):
        return np.array([(u >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)

    seen = set()
    for u1 in cc.gpart_u1s(oracle_lib):
        g, ref = np.zeros(17, np.int32), np.zeros(17, np.int32)
        VB.h_vb_gdigits(words(u1).ctypes.data, g.ctypes.data, ref.ctypes.data)
        assert g.tolist() == ref.tolist() == cc.gdigits(u1), hex(u1)
        seen.update((i, d) for i, d in enumerate(g.tolist()))
    assert all((w, d) in seen for w in range(16) for d in (1, -1, 2, 32767, 32768, -32767))
    assert (16, 1) in seen and (15, 0) in seen and (15, -1) in seen
    for _, u2 in cc.ladder_scalars():
        d = np.zeros(65, np.int32)
        VB.h_vb_digits(words(u2).ctypes.data, d.ctypes.data)
        assert d.tolist() == [x for x, _ in cc.signed_digits(u2, [4] * 65)], hex(u2)


@pytest.mark.parametrize("fam", ["ladder", "gpart", "keyshape"])
def test_family_bits_and_rerun(VB, gtab, oracle_lib, fam):
    """accept bits == the oracle's; the exact rerun ran exactly where it is
    pinned on (u2 = n - 2 under every key; every built G-part meeting) and
    nowhere it is pinned off"""
    h, s, xy, want, names, rerun, _ = cc.family(oracle_lib, fam)
    got, ran = vb_run(VB, gtab, h, s, xy)
    assert not named(names, got != want)
    pinned = np.array([r is not None for r in rerun])
    on = np.array([bool(r) for r in rerun])
    assert not named(names, pinned & (ran != on))
    assert pinned.sum() >= len(h) // 2
    if fam == "ladder":
        assert [n for n, r in zip(names, rerun) if r] == ["ladder: u2 = n - 2 under %s" % k[0] for k in cc.keys()]
    if fam == "gpart":
        assert on.sum() == 5 * (9 + 7) and want[on].sum() == 5 * 7
    if fam == "keyshape":
        assert not ran.any()


def test_sec1_decode_and_bits(S1, gtab, oracle_lib):
    """h_sec1_decode == Python's decode for every key of the sweep, accepted
    or not; then the verify under the decoded key, in every format"""
    h, s, xy, want, names, _, _ = cc.family(oracle_lib, "sec1")
    comp = wc.encode(xy, KEY_COMPRESSED)
    py_xy, py_ok = wc.decoded_xy(comp, KEY_COMPRESSED)
    got_xy, got_ok = s1_decode(S1, comp, KEY_COMPRESSED)
    assert not named(names, got_ok != py_ok)
    assert not named(names, (got_xy != py_xy).any(axis=1))
    assert (py_ok == want).all() and 0.4 * len(h) <= py_ok.sum() <= 0.6 * len(h)
    assert (py_xy[py_ok] == xy[py_ok]).all()
    for fmt in (KEY_COMPRESSED, KEY_UNCOMPRESSED, KEY_XY):
        keys, w = cc.wire(oracle_lib, h, s, xy, fmt)
        assert (w == want).all()
        assert not named(names, s1_run(S1, gtab, h, s, keys, fmt) != w)
        if fmt != KEY_COMPRESSED:  # a key without a point is off the curve as X||Y too
            _, ok = s1_decode(S1, keys, fmt)
            assert (ok == py_ok).all()


@pytest.mark.parametrize("order", ["natural", "permuted"])
def test_combined_both_orders(VB, S1, gtab, oracle_lib, order):
    c = cc.combined(oracle_lib)
    h, s, xy, want, idx = cc.ordered(c, order)
    names = [c["names"][i] for i in idx]
    got, ran = vb_run(VB, gtab, h, s, xy)
    assert not named(names, got != want)
    keys, w = cc.wire(oracle_lib, h, s, xy, KEY_COMPRESSED)
    assert (w == want).all()  # (every rejected key here is rejected in either form)
    assert not named(names, s1_run(S1, gtab, h, s, keys, KEY_COMPRESSED) != w)
    sizes = {f: c["family"].count(f) for f in cc.FAMILIES}
    assert sum(sizes.values()) == len(want) and all(v >= 100 for v in sizes.values()), sizes


def write_dump(path, oracle_lib):
    c = cc.combined(oracle_lib)
    h, s, xy, want, _ = cc.ordered(c, "natural")
    comp, want_c = cc.wire(oracle_lib, h, s, xy, KEY_COMPRESSED)
    cxy, cok = wc.decoded_xy(comp, KEY_COMPRESSED)
    rerun = np.array([255 if r is None else int(r) for r in c["rerun"]], np.uint8)
    with open(path, "wb") as f:
        f.write(b"CARRIED1" + struct.pack("<Q", len(h)))
        for a in (h, s, xy, comp, want.astype(np.uint8), want_c.astype(np.uint8), rerun, cok.astype(np.uint8), cxy):
            f.write(np.ascontiguousarray(a, np.uint8).tobytes())
    return len(h), int((~cok).sum()), int((rerun == 1).sum())


@pytest.mark.parametrize("which", ["varbase", "sec1"])
def test_stand_alone_programs_walk_the_set_under_sanitizers(oracle_lib, tmp_path, which):
    """host code only, each program its own process: any sanitizer report
    aborts it, any bit that differs from the dump fails it"""
    dump = str(tmp_path / "carried.bin")
    n, rejected, reruns = write_dump(dump, oracle_lib)
    src, exe = os.path.join(_CPP, which + "_harness.cpp"), os.path.join(_CPP, which + "_san")
    if _stale(exe, src):
        subprocess.run(["g++"] + _SAN + ["-D%s_MAIN" % which.upper(), "-o", exe, src], check=True)
    p = subprocess.run([exe, "0", dump], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    tail = "%d reruns" % reruns if which == "varbase" else "%d keys rejected" % rejected
    assert "carried: 0 mismatches of %d (%s)" % (n, tail) in p.stdout, p.stdout
