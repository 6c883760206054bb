"""The signer on the CPU: simple_pbft_amd/csrc/sign.h (the limb code the sign
kernels run) and der.h's writer compiled with g++ (tests/cpp/sign_harness.cpp),
every output byte compared with tests/rfc6979_model.py over the case lists of
tests/sign_cases.py.  The same harness, built as a stand-alone program with the
address and undefined-behaviour sanitizers, is run once."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rfc6979_model as model
import sign_cases as sc
from conftest import ROOT
from oracle import der as oder
from oracle import p256

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "sign_harness.cpp")
_CSRC = os.path.join(ROOT, "simple_pbft_amd", "csrc")
_HDRS = [os.path.join(_CSRC, f) for f in ("sign.h", "sha256_block.h", "der.h", "varbase.h", "p256_algo.h", "fe29.h",
                                          "fes.h", "safegcd.h", "p256_consts.h")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [_SRC])


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libsign_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.h_sg_g_table_words.restype = u64
    lib.h_sg_build_g_table.argtypes = [vp]
    lib.h_sg_drbg.argtypes = [vp, vp, ctypes.c_int, vp]
    lib.h_sg_sign_with_k.argtypes = [u64, vp, vp, vp, vp, vp, vp, vp]
    lib.h_sg_x_mod_n.argtypes = [vp, vp]
    lib.h_sg_key_ok.argtypes = [vp]
    lib.h_sg_sign.argtypes = [u64, vp, vp, vp, vp, vp]
    lib.h_sg_der_from_rs.argtypes = [vp, vp]
    lib.h_sg_der_from_rs.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def gtab(H):
    """the width-16 comb table of G (34 MiB), built once by p256_algo.h's serial builder"""
    t = np.zeros(H.h_sg_g_table_words(), np.uint32)
    H.h_sg_build_g_table(t.ctypes.data)
    return t


def sign_rows(H, gtab, hashes, ds):
    hashes, ds = np.ascontiguousarray(hashes, np.uint8), np.ascontiguousarray(ds, np.uint8)
    n = len(hashes)
    rs, ok = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8)
    H.h_sg_sign(n, hashes.ctypes.data, ds.ctypes.data, gtab.ctypes.data, rs.ctypes.data, ok.ctypes.data)
    return rs, ok.astype(bool)


def test_rfc_rows_through_the_limb_code(H, gtab, ecdsa_fixtures):
    d = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    hs = [hashlib.sha256(m).digest() for m in (b"sample", b"test")]
    rs, ok = sign_rows(H, gtab, np.frombuffer(b"".join(hs), np.uint8).reshape(2, 32), sc.col([d, d]))
    by_hash = {v["hash"]: v for v in ecdsa_fixtures["vectors"] if v["kind"].startswith("rfc6979") and v["expect"]}
    assert ok.all()
    for i, h in enumerate(hs):
        assert rs[i].tobytes().hex() == by_hash[h.hex()]["r"] + by_hash[h.hex()]["s"]


def test_drbg_first_three_candidates(H):
    """rfc6979_init / rfc6979_next at the bits2octets seam crossed with the ends
    of the key range, and on 64 random pairs: three candidates each, so the
    between-candidates update runs twice."""
    cases = sc.drbg_cases()
    assert len(cases) == 24 + 64
    want = sc.drbg_expected(cases, 3)
    got = np.zeros_like(want)
    for i, (d, h) in enumerate(cases):
        db, hb = sc.col([d]), sc.col([h])
        H.h_sg_drbg(db.ctypes.data, hb.ctypes.data, 3, got[i].ctypes.data)
    assert (got == want).all(), np.nonzero((got != want).any(axis=(1, 2)))[0]
    # h1 = n and h1 = 0 are one input after bits2octets; h1 = n + 1 and 1 likewise
    by = {c: got[i] for i, c in enumerate(cases)}
    assert (by[(1, sc.N)] == by[(1, 0)]).all() and (by[(1, sc.N + 1)] == by[(1, 1)]).all()
    assert not (by[(1, sc.N - 1)] == by[(1, 0)]).all()


def test_sign_with_chosen_k(H, gtab):
    """ecdsa_sign_with_k over the chosen nonces -- range ends, single windows,
    the recoding-carry seam alone and in runs to the top window, all ones --
    crossed with e in {0, n-1, n, 2^256-1} and d in {1, n-1}: byte for byte the
    model's (r, s), each accepted by oracle.p256.verify; no rerun is taken."""
    cases = sc.with_k_cases()
    want_rs, want_ok = sc.with_k_expected()
    e, d, k = (sc.col([c[j] for c in cases]) for j in range(3))
    n = len(cases)
    rs, ok, paths = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    H.h_sg_sign_with_k(n, e.ctypes.data, d.ctypes.data, k.ctypes.data, gtab.ctypes.data, rs.ctypes.data,
                       ok.ctypes.data, paths.ctypes.data)
    assert (ok.astype(bool) == want_ok).all()
    assert (rs == want_rs).all(), np.nonzero((rs != want_rs).any(axis=1))[0]
    assert want_ok.all()  # (no chosen case has r = 0 or s = 0)
    assert not paths.any()
    pub = {dd: p256.pubkey(dd) for dd in sc.D_PAIR}
    for i, (ee, dd, _) in enumerate(cases):
        r, s = int.from_bytes(rs[i, :32].tobytes(), "big"), int.from_bytes(rs[i, 32:].tobytes(), "big")
        assert p256.verify(sc.be(ee), r, s, *pub[dd]), i


def test_sign_with_k_refuses_k_out_of_range(H, gtab):
    ks = [0, sc.N, sc.N + 1, sc.TOP]
    n = len(ks)
    e, d, k = sc.col([5] * n), sc.col([7] * n), sc.col(ks)
    rs, ok = np.full((n, 64), 0xEE, np.uint8), np.ones(n, np.uint8)
    H.h_sg_sign_with_k(n, e.ctypes.data, d.ctypes.data, k.ctypes.data, gtab.ctypes.data, rs.ctypes.data,
                       ok.ctypes.data, None)
    assert not ok.any() and not rs.any()


def test_x_mod_n_reduction(H):
    """r = x mod n on its own: no nonce with R.x in [n, p) can be found (2^-128
    of all x), so no whole signature reaches the subtraction."""
    for x in sc.X_MOD_N:
        xb, out = sc.col([x]), np.zeros(32, np.uint8)
        H.h_sg_x_mod_n(xb.ctypes.data, out.ctypes.data)
        assert int.from_bytes(out.tobytes(), "big") == x % sc.N, hex(x)


def test_sign_end_to_end_random(H, gtab):
    pairs = sc.random_pairs(256)
    hashes = np.frombuffer(b"".join(h for h, _ in pairs), np.uint8).reshape(-1, 32)
    rs, ok = sign_rows(H, gtab, hashes, sc.col([d for _, d in pairs]))
    assert ok.all()
    want = sc.sign_expected(pairs)
    assert (rs == want).all(), np.nonzero((rs != want).any(axis=1))[0]


def test_invalid_private_keys_are_refused(H, gtab):
    for d in sc.BAD_KEYS:
        assert H.h_sg_key_ok(sc.col([d]).ctypes.data) == 0
    for d in (1, sc.N - 1):
        assert H.h_sg_key_ok(sc.col([d]).ctypes.data) == 1
    n = len(sc.BAD_KEYS)
    rs, ok = sign_rows(H, gtab, sc.col([9] * n), sc.col(sc.BAD_KEYS))
    assert not ok.any() and not rs.any()


def _der(H, rs_row):
    slot = np.full(72, 0xEE, np.uint8)
    ln = H.h_sg_der_from_rs(np.ascontiguousarray(rs_row).ctypes.data, slot.ctypes.data)
    return slot, ln


def test_der_writer_on_the_searched_shapes(H, gtab):
    """der_from_rs on signatures whose r or s has a zero top byte (followed by a
    byte with its top bit clear, and set), two zero top bytes, the top bit set,
    and the shortest / longest encodings the search met: equal to
    oracle/der.py's encoding, and back through the product's parser."""
    from simple_pbft_amd import pbftv
    L = pbftv.lib()
    cases = sc.der_fixture()
    names = {c["name"] for c in cases}
    assert {"r_zero_byte_then_clear", "s_zero_byte_then_clear", "r_zero_byte_then_top_bit",
            "s_zero_byte_then_top_bit", "r_two_zero_bytes", "s_two_zero_bytes", "both_top_bits_set_72",
            "neither_top_bit_70", "shortest_met"} <= names
    lens = set()
    for c in cases:
        h, d = bytes.fromhex(c["hash"]), int(c["d"], 16)
        want_rs = model.sign_bytes(h, d)
        rs, ok = sign_rows(H, gtab, np.frombuffer(h, np.uint8).reshape(1, 32), sc.col([d]))
        assert ok.all() and rs[0].tobytes() == want_rs, c["name"]
        r, s = int.from_bytes(want_rs[:32], "big"), int.from_bytes(want_rs[32:], "big")
        shape = c["name"]
        if shape.startswith(("r_zero_byte", "r_two")):
            assert want_rs[0] == 0 and (want_rs[1] == 0) == ("two" in shape)
        if shape.startswith(("s_zero_byte", "s_two")):
            assert want_rs[32] == 0 and (want_rs[33] == 0) == ("two" in shape)
        slot, ln = _der(H, rs[0])
        enc = oder.encode(r, s)
        assert ln == len(enc) == c["der_len"] and slot[:ln].tobytes() == enc and not slot[ln:].any(), c["name"]
        back = np.zeros(64, np.uint8)
        assert L.pbftv_ecdsa_der_to_rs(slot[:ln].tobytes(), ln, back.ctypes.data) == 1
        assert back.tobytes() == want_rs
        lens.add(ln)
    assert min(lens) == 68 and max(lens) == 72


def test_der_writer_on_crafted_integers(H):
    """Integer shapes no signature search reaches: zero, one byte, every count
    of leading zero bytes, with the first kept byte at 0x7f / 0x80."""
    vals = [0, 1, 0x7F, 0x80, 0xFF, sc.N - 1, sc.TOP, 1 << 255, (1 << 255) - 1]
    for z in range(1, 32):
        vals += [0x7F << (8 * (31 - z)), 0x80 << (8 * (31 - z))]
    for r in vals:
        for s in (vals[3], vals[-1], r):
            rs = np.frombuffer(sc.be(r) + sc.be(s), np.uint8)
            slot, ln = _der(H, rs)
            enc = oder.encode(r, s)
            assert ln == len(enc) and slot[:ln].tobytes() == enc and not slot[ln:].any(), (hex(r), hex(s))
            assert oder.to_rs(slot[:ln].tobytes()) == rs.tobytes()


def test_stand_alone_program_under_sanitizers():
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only): the same entry points on heap buffers of exactly the
    documented sizes -- the 72-byte DER slots among them -- against the RFC's
    rows; any sanitizer report aborts it."""
    exe = os.path.join(_CPP, "sign_san")
    if _stale(exe):
        # (shift-base off: fe29.h's carry folds shift negative limbs left on
        # purpose -- two's complement, what the GPU does and C++20 defines)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize=shift-base",
                        "-fno-sanitize-recover=all", "-DSIGN_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sign: 0 mismatches" in p.stdout
