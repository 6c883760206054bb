"""The sealed wire forms' arithmetic on the CPU (simple_pbft_amd/csrc/wire.h
with gojson_enc.h, compiled by g++ as tests/cpp/wire_harness.cpp): the length
k_seal_lengths computes -- preimage length plus signature tails -- equals the
length of oracle/gojson.py's *_signed form for every kind, the *_signed
encoders fill exactly that many bytes through a bounded sink, the documented
upper bounds hold, and the offsets' host reference equals numpy.cumsum.  The
same harness runs once as a stand-alone program under the address and
undefined-behaviour sanitizers."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import seal_cases as cases
from conftest import ROOT
from oracle import gojson

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "wire_harness.cpp")
_HDRS = [os.path.join(ROOT, "simple_pbft_amd", "csrc", f) for f in ("wire.h", "gojson_enc.h")]
u64, i64, cp = ctypes.c_uint64, ctypes.c_int64, ctypes.c_char_p
_OUT = [ctypes.c_void_p, u64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in _HDRS + [_SRC])


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libwire_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.h_wire_vote.restype = lib.h_wire_reply.restype = lib.h_wire_preprepare.restype = u64
    lib.h_wire_vote.argtypes = [i64, i64, cp, u64, cp, u64, i64, cp, u64] + _OUT
    lib.h_wire_reply.argtypes = [i64, i64, cp, u64, cp, u64, cp, u64, cp, u64] + _OUT
    lib.h_wire_preprepare.argtypes = [i64, i64, cp, u64, ctypes.c_int, i64, cp, u64, cp, u64, i64, cp, u64,
                                      ctypes.c_int, cp, u64] + _OUT
    lib.h_wire_scan.restype = u64
    lib.h_wire_scan.argtypes = [ctypes.c_void_p, u64, ctypes.c_void_p]
    lib.h_wire_scan_block.restype = lib.h_wire_scan_chunk.restype = ctypes.c_uint32
    return lib


def run(H, kind, msg, req_sig, sig):
    """(wire.h's length, the encoder's bytes through the bounded sink, bytes
    that fell past the length, wire.h's bound with this signature length)"""
    cap = 4096
    out = ctypes.create_string_buffer(cap)
    wr, ov, bd = u64(), u64(), u64()
    tail = [sig, len(sig), out, cap, ctypes.byref(wr), ctypes.byref(ov), ctypes.byref(bd)]
    if kind == "vote":
        view, seq, dg, nid, mt = msg
        ln = H.h_wire_vote(view, seq, dg, len(dg), nid, len(nid), mt, *tail)
    elif kind == "reply":
        view, ts, cid, nid, res = msg
        ln = H.h_wire_reply(view, ts, cid, len(cid), nid, len(nid), res, len(res), *tail)
    else:
        view, seq, dg, req = msg
        rts, rcid, rop, rseq = req if req is not None else (0, b"", b"", 0)
        ln = H.h_wire_preprepare(view, seq, dg, len(dg), req is not None, rts, rcid, len(rcid), rop, len(rop), rseq,
                                 req_sig or b"", len(req_sig or b""), req_sig is None, *tail)
    assert ln <= cap
    return ln, out.raw[:min(wr.value, ln)], wr.value, ov.value, bd.value


def _cases(kind):
    """the distinct cases crossed with every signature length; a pre-prepare's
    client signature runs through nil and every length against each of them"""
    rng = np.random.default_rng(0xC0DE)
    for i, (msg, _) in enumerate(cases.distinct(kind)):
        for j, n in enumerate(cases.SIG_LENS):
            sig = rng.bytes(n)
            if kind != "preprepare":
                yield msg, None, sig
                continue
            k = (i + j) % (len(cases.SIG_LENS) + 1)
            yield msg, (None if k == len(cases.SIG_LENS) else rng.bytes(cases.SIG_LENS[k])), sig


@pytest.mark.parametrize("kind", cases.KINDS)
def test_length_bytes_and_bound_match_the_oracle(H, kind):
    seen_req, seen_nil, seen_pads = set(), set(), set()
    for msg, req_sig, sig in _cases(kind):
        want = cases.wire(kind, msg, req_sig, sig)
        ln, got, written, over, bound = run(H, kind, msg, req_sig, sig)
        assert ln == len(want), (msg, req_sig, sig)
        assert written == ln and over == 0 and got == want
        assert bound >= ln
        seen_pads.add(len(sig) % 3)
        if kind == "preprepare":
            seen_req.add(msg[3] is not None)
            if msg[3] is not None:
                seen_nil.add(None if req_sig is None else len(req_sig))
    assert seen_pads == {0, 1, 2}
    if kind == "preprepare":
        assert seen_req == {False, True} and seen_nil == {None, *cases.SIG_LENS}


def test_cases_cover_the_families():
    for kind in cases.KINDS:
        ints, strs = set(), set()
        for msg, _ in cases.distinct(kind):
            flat = list(msg[:3]) + (list(msg[3]) if kind == "preprepare" and msg[3] is not None else list(msg[3:]))
            ints |= {x for x in flat if isinstance(x, int)}
            strs |= {x for x in flat if isinstance(x, bytes)}
        assert {cases.I64_MIN, cases.I64_MAX, 0, -1} <= ints
        assert b"" in strs
        joined = b"|".join(strs)
        for part in cases.PARTS:
            assert part in joined


def test_header_states_the_bounds_wire_h_computes(H):
    """include/pbftv.h's closed forms -- 120 / 102 / 189 + 6 x string bytes + T,
    T = 103 or 111, + 15 + 4 ceil(req_sig_len / 3) -- against wire.h's."""
    with open(os.path.join(ROOT, "include", "pbftv.h")) as f:
        hdr = f.read()
    assert re.search(r"T = 103 \(PBFTV_SIG_RS\) or 111\s+\*?\s*\(PBFTV_SIG_DER\)", hdr)
    for base in ("vote         120 + 6", "reply        102 + 6", "pre-prepare  189 + 6", "+ T + 15 + 4 ceil"):
        assert base in hdr
    for sig_max, t in ((64, 103), (72, 111)):
        sig = bytes(sig_max)
        for a, b, c, rs in ((0, 0, 0, 0), (1, 2, 3, 1), (64, 5, 17, 72), (70, 70, 70, 80)):
            sa, sb, sc_ = b"\x00" * a, b"\x01" * b, b"\xff" * c
            m = cases.I64_MIN
            assert run(H, "vote", (m, m, sa, sb, m), None, sig)[4] == 120 + 6 * (a + b) + t
            assert run(H, "reply", (m, m, sa, sb, sc_), None, sig)[4] == 102 + 6 * (a + b + c) + t
            assert (run(H, "preprepare", (m, m, sa, (m, sb, sc_, m)), bytes(rs), sig)[4] ==
                    189 + 6 * (a + b + c) + t + 15 + 4 * ((rs + 2) // 3))
            # the all-sixfold message with minimal integers' widths reaches the bound but for the braces' slack
            ln = run(H, "vote", (m, m, sa, sb, m), None, sig)[0]
            assert ln <= 120 + 6 * (a + b) + t and ln >= 6 * (a + b) + t


def test_scan_reference_equals_cumsum(H):
    rng = np.random.default_rng(0x5CA7)
    for n in (0, 1, 2, 255, 256, 257, 5000):
        ln = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        ln[rng.integers(0, 3, n) == 0] = 0
        off = np.full(n + 1, 0xEE, np.uint64)
        total = H.h_wire_scan(ln.ctypes.data, n, off.ctypes.data)
        want = np.cumsum(ln.astype(np.uint64), dtype=np.uint64)
        assert total == (int(want[-1]) if n else 0) and off[n] == 0xEE
        assert off[:n].tolist() == ([0] + want[:-1].tolist() if n else [])
        if n == 5000:
            assert total > 2 ** 32 and (ln == 0).any()
    assert H.h_wire_scan_block() == 256 and H.h_wire_scan_chunk() == 256


def test_oracle_signed_forms_extend_their_preimages():
    """what the arithmetic rests on: the signed form is the preimage without its
    closing brace, then the signature field"""
    for kind in cases.KINDS:
        for msg, req_sig in cases.distinct(kind)[:16]:
            pre = cases.preimage(kind, msg)
            w = cases.wire(kind, msg, None if kind != "preprepare" else None, b"abc")
            if kind != "preprepare" or msg[3] is None:
                assert w == pre[:-1] + b',"signature":"YWJj"}'
            else:
                assert w == pre[:-2] + b',"signature":null},"signature":"YWJj"}'
    assert gojson.vote_signed(0, 0, b"", b"", 0, b"") .endswith(b',"signature":""}')


def test_stand_alone_program_under_sanitizers():
    exe = os.path.join(_CPP, "wire_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DWIRE_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "wire: 0 mismatches" in p.stdout
