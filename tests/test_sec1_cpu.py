"""Keys in SEC1 wire form on the CPU: simple_pbft_amd/csrc/sec1.h (the limb code
k_varbase_keys_sec1 runs) compiled with g++ (tests/cpp/sec1_harness.cpp) and
checked against Python big integers -- fe_sqrt_p against pow(t, (p+1)/4, p),
sec1_key_check against tests/wirekey_cases.decode -- then one end-to-end pass:
the decoded keys through varbase.h's verify over the vectors of
varbase_cases.all_vectors re-encoded in both formats, against the oracle.  The
same harness, built as a stand-alone program with the address and
undefined-behaviour sanitizers, is run once."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import varbase_cases as vc
import wirekey_cases as wc
from conftest import ROOT
from wirekey_cases import B, GX, GY, KEY_COMPRESSED, KEY_UNCOMPRESSED, KEY_XY, P

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "sec1_harness.cpp")
_CSRC = os.path.join(ROOT, "simple_pbft_amd", "csrc")
_HDRS = [os.path.join(_CSRC, f) for f in ("sec1.h", "varbase.h", "p256_algo.h", "fe29.h", "fes.h", "safegcd.h",
                                          "p256_consts.h")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [_SRC])


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libsec1_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.h_sec1_key_bytes.restype = ctypes.c_uint32
    lib.h_sec1_key_bytes.argtypes = [ctypes.c_int]
    lib.h_sec1_sqrt.argtypes = [ctypes.c_uint64, vp, vp, vp]
    lib.h_sec1_decode.argtypes = [ctypes.c_uint64, vp, ctypes.c_int, vp, vp]
    lib.h_sec1_g_table_words.restype = ctypes.c_uint64
    lib.h_sec1_build_g_table.argtypes = [vp]
    lib.h_sec1_verify_batch.argtypes = [ctypes.c_uint64, vp, vp, vp, ctypes.c_int, vp, vp]
    return lib


def sqrt_batch(H, ts):
    t = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in ts), np.uint8).copy()
    y, ok = np.zeros(32 * len(ts), np.uint8), np.zeros(len(ts), np.uint8)
    H.h_sec1_sqrt(len(ts), t.ctypes.data, y.ctypes.data, ok.ctypes.data)
    return [int.from_bytes(y[32 * i:32 * i + 32].tobytes(), "big") for i in range(len(ts))], ok.astype(bool).tolist()


def decode_batch(H, keys: list, fmt: int):
    """[(x, y) or None] by sec1_key_check"""
    k = np.frombuffer(b"".join(keys), np.uint8).copy()
    assert len(k) == wc.STRIDE[fmt] * len(keys)
    xy, ok = np.zeros(64 * len(keys), np.uint8), np.zeros(len(keys), np.uint8)
    H.h_sec1_decode(len(keys), k.ctypes.data, fmt, xy.ctypes.data, ok.ctypes.data)
    out = []
    for i in range(len(keys)):
        b = xy[64 * i:64 * i + 64].tobytes()
        out.append((int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")) if ok[i] else None)
    return out


def test_key_bytes(H):
    assert [H.h_sec1_key_bytes(f) for f in (0, 1, 2, 3, -1)] == [64, 33, 65, 0, 0]


def test_sqrt_against_python(H):
    with_root, without = (0, 5, 6, 8, 9, P - 3, P - 4), (1, 2, 3, 4, 7, P - 1, P - 2)
    assert all(wc.sqrt_p(wc.rhs(x))[1] for x in with_root) and not any(wc.sqrt_p(wc.rhs(x))[1] for x in without)
    rng = np.random.default_rng(2024)
    ts = [0, 1, 4, B, P - 1] + [wc.rhs(x) for x in with_root + without]
    ts += [int.from_bytes(rng.bytes(32), "big") % P for _ in range(2000)]
    ys, oks = sqrt_batch(H, ts)
    want = [wc.sqrt_p(t) for t in ts]
    bad = [hex(t) for t, y, ok, (wy, wok) in zip(ts, ys, oks, want) if ok != wok or y != wy]
    assert not bad, bad[:4]
    assert oks[:5] == [True, True, True, wc.sqrt_p(B)[1], False]  # (p - 1 is no square: p == 3 mod 4)
    assert oks[5:5 + len(with_root)] == [True] * len(with_root)
    assert oks[5 + len(with_root):5 + len(with_root) + len(without)] == [False] * len(without)
    assert any(oks[-2000:]) and not all(oks[-2000:])
    assert all(y * y % P == t for t, y, ok in zip(ts, ys, oks) if ok)


def test_compressed_keys(H):
    valid = [k for k, v in wc.golden_keys() if v]
    assert len(valid) >= 4
    for xy in valid:
        x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")
        right, wrong = wc.encode_one(xy, KEY_COMPRESSED), wc.encode_one(xy, KEY_COMPRESSED, wrong_parity=True)
        assert decode_batch(H, [right, wrong], KEY_COMPRESSED) == [(x, y), (x, P - y)]
        assert wc.decode(right, KEY_COMPRESSED) == (x, y) and wc.decode(wrong, KEY_COMPRESSED) == (x, P - y)
    # G itself: the published Gy, which is odd
    g = GX.to_bytes(32, "big")
    assert decode_batch(H, [b"\x03" + g, b"\x02" + g], KEY_COMPRESSED) == [(GX, GY), (GX, P - GY)]
    # X out of range, foreign prefixes
    assert decode_batch(H, [b"\x02" + P.to_bytes(32, "big"), b"\x03" + P.to_bytes(32, "big"),
                            b"\x02" + b"\xff" * 32, b"\x03" + b"\xff" * 32], KEY_COMPRESSED) == [None] * 4
    pres = (0x00, 0x01, 0x04, 0x05, 0x06, 0x07, 0xFF)
    assert decode_batch(H, [bytes([p]) + g for p in pres], KEY_COMPRESSED) == [None] * len(pres)
    # small and random X, both prefixes, against the Python decode
    rng = np.random.default_rng(7)
    xs = list(range(0, 12)) + [P - 1, P - 2, P - 3, P - 4] + [int.from_bytes(rng.bytes(32), "big") % P
                                                              for _ in range(300)]
    keys = [bytes([pre]) + x.to_bytes(32, "big") for x in xs for pre in (2, 3)]
    got, want = decode_batch(H, keys, KEY_COMPRESSED), [wc.decode(k, KEY_COMPRESSED) for k in keys]
    assert got == want
    assert any(w is None for w in want) and any(w is not None for w in want)
    assert all(w is None or (wc.on_curve(*w) and (w[1] & 1) == (k[0] & 1)) for w, k in zip(want, keys))


def test_uncompressed_and_xy_keys(H):
    gold = wc.golden_keys()
    assert any(not v for _, v in gold)
    for xy, v in gold:
        x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")
        want = (x, y) if v else None
        assert wc.decode(b"\x04" + xy, KEY_UNCOMPRESSED) == want  # (the fixture's verdicts are Python's)
        assert decode_batch(H, [b"\x04" + xy], KEY_UNCOMPRESSED) == [want]
        assert decode_batch(H, [xy], KEY_XY) == [want]
    xy = next(k for k, v in gold if v)
    pres = (0x00, 0x02, 0x03, 0x06, 0x07)
    assert decode_batch(H, [bytes([p]) + xy for p in pres], KEY_UNCOMPRESSED) == [None] * len(pres)
    x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")
    bad = [b"\x04" + xy[:32] + P.to_bytes(32, "big"), b"\x04" + xy[:32] + b"\xff" * 32,
           b"\x04" + P.to_bytes(32, "big") + xy[32:], b"\x04" + xy[:32] + ((y + 1) % P).to_bytes(32, "big")]
    assert decode_batch(H, bad, KEY_UNCOMPRESSED) == [None] * len(bad)
    assert decode_batch(H, [b"\x04" + wc.xy_bytes(x, P - y)], KEY_UNCOMPRESSED) == [(x, P - y)]


def test_rejected_set_against_python(H, oracle_lib):
    """the set the GPU tests spread over their waves: sec1_key_check == Python, case by case"""
    _, _, _, cases = wc.rejected_set(oracle_lib)
    for fmt in (KEY_COMPRESSED, KEY_UNCOMPRESSED):
        mine = [(n, k) for n, f, k in cases if f == fmt]
        got = decode_batch(H, [k for _, k in mine], fmt)
        wrong = [n for (n, k), g in zip(mine, got) if g != wc.decode(k, fmt)]
        assert not wrong, wrong
        assert any(g is None for g in got) and any(g is not None for g in got)


def test_end_to_end_against_the_oracle(H, oracle_lib):
    """sec1_key_check, stage 1, varbase_verify over all_vectors in both SEC1
    formats; a key that is no point stays a rejection in either (compressed:
    rejected, or decoded to a point the signature was not made under)."""
    gtab = np.zeros(H.h_sec1_g_table_words(), np.uint32)
    H.h_sec1_build_g_table(gtab.ctypes.data)
    h, s, p, want_xy = vc.all_vectors(oracle_lib)
    for fmt in (KEY_COMPRESSED, KEY_UNCOMPRESSED):
        keys = wc.encode(p, fmt)
        want = wc.expect(oracle_lib, h, s, keys, fmt)
        if fmt == KEY_UNCOMPRESSED:
            assert (want == want_xy).all()
        assert want.any() and not want.all()
        out = np.zeros(len(h), np.uint8)
        H.h_sec1_verify_batch(len(h), h.ctypes.data, s.ctypes.data, keys.ctypes.data, fmt, gtab.ctypes.data,
                              out.ctypes.data)
        assert (out.astype(bool) == want).all(), np.nonzero(out.astype(bool) != want)[0]


def test_stand_alone_program_under_sanitizers():
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only): k G for k <= 64 and random X decoded in every format and
    parity; any sanitizer report aborts it."""
    exe = os.path.join(_CPP, "sec1_san")
    if _stale(exe):
        # (shift-base off: fe29.h's carry folds shift negative limbs left on
        # purpose -- two's complement, what the GPU does and C++20 defines)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                        "-fno-sanitize-recover=all", "-DSEC1_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe, "128"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sec1: 0 mismatches" in p.stdout
