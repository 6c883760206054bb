"""DER signatures on the CPU: simple_pbft_amd/csrc/der.h (the parser
k_der_to_rs runs) compiled with g++ (tests/cpp/der_harness.cpp) and checked
against oracle/der.py -- the whole corpus of tests/der_cases.py behind the
host's pointer reader and behind the kernel's dword reader (whose every fetch
is checked against the kernel's read rule), every 1- and 2-byte mutation of
the header bytes of one valid encoding, the 72-byte fact the kernel is built
on, and the same parse in a stand-alone program under the address and
undefined-behaviour sanitizers with every encoding in a heap block of exactly
its size."""
from __future__ import annotations

import ctypes
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import der_cases as dc
from conftest import ROOT
from oracle import der as oder

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "der_harness.cpp")
_HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "der.h")


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in (_HDR, _SRC))


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libder_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.h_der_ptr.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp]
    lib.h_der_probe.argtypes = [ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
    lib.h_der_dwords.restype = ctypes.c_uint64
    lib.h_der_dwords.argtypes = [ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, vp]
    return lib


def pack(ders):
    ln = np.array([len(d) for d in ders], np.uint32)
    off = np.zeros(len(ders), np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(ders) + b"\x00", np.uint8).copy(), off, ln


def run_ptr(H, blob, off, ln):
    n = len(ln)
    rs, ok = np.full((n, 64), 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    H.h_der_ptr(n, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, rs.ctypes.data, ok.ctypes.data)
    return rs, ok.astype(bool)


def run_probe(H, blob, off, ln):
    n = len(ln)
    rs, ok, mx = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int64)
    H.h_der_probe(n, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, rs.ctypes.data, ok.ctypes.data, mx.ctypes.data)
    return rs, ok.astype(bool), mx


def run_dwords(H, blob, off, ln):
    n = len(ln)
    rs, ok = np.full((n, 64), 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    bad = H.h_der_dwords(n, blob.ctypes.data, len(blob), off.ctypes.data, ln.ctypes.data, rs.ctypes.data,
                         ok.ctypes.data)
    return rs, ok.astype(bool), bad


def oracle_rs(ders):
    rs, ok = np.zeros((len(ders), 64), np.uint8), np.zeros(len(ders), bool)
    for i, d in enumerate(ders):
        w = oder.to_rs(d)
        if w is not None:
            rs[i], ok[i] = np.frombuffer(w, np.uint8), True
    return rs, ok


def check_all_readers(H, ders):
    """the three readers against the oracle on packed encodings; returns parsed"""
    want_rs, want_ok = oracle_rs(ders)
    blob, off, ln = pack(ders)
    rs, ok = run_ptr(H, blob, off, ln)
    assert (ok == want_ok).all(), [ders[i].hex() for i in np.nonzero(ok != want_ok)[0][:4]]
    assert (rs == want_rs).all()
    rs, ok, mx = run_probe(H, blob, off, ln)
    assert (ok == want_ok).all() and (rs == want_rs).all()
    assert (mx < np.minimum(ln, 72)).all()
    rs, ok, bad = run_dwords(H, blob, off, ln)
    assert (ok == want_ok).all() and (rs == want_rs).all()
    assert bad == 0
    return want_ok


@pytest.fixture(scope="module")
def corpora(oracle_lib):
    return {"registered": dc.registered_corpus(oracle_lib)[-1], "carried": dc.carried_corpus(oracle_lib)[-1]}


@pytest.mark.parametrize("which", ["registered", "carried"])
def test_corpus_against_the_oracle(H, oracle_lib, corpora, which):
    corpus = corpora[which]
    bits = (dc.registered_batch if which == "registered" else dc.carried_batch)(oracle_lib, len(corpus))[-1]
    dc.check_corpus(corpus, bits)
    ok = check_all_readers(H, [c.der for c in corpus])
    assert ok.any() and not ok.all()
    assert all(ok[i] for i, c in enumerate(corpus) if c.valid_class)
    assert not any(ok[i] for i, c in enumerate(corpus) if not c.valid_class)


@pytest.mark.parametrize("seed,tight", [(1, True), (2, True), (3, False)])
def test_corpus_as_the_tests_place_it(H, oracle_lib, corpora, seed, tight):
    """shuffled, at every offset modulo 16, sharing bytes, truncated encodings
    followed by their missing bytes, a 72-byte encoding claimed as 10,000 and
    as 2^32 - 1 bytes long: r||s and parsed equal the oracle's behind every
    reader, and the dword reader fetches nothing outside the rule"""
    cases = dc.with_claim(dc.with_claim(dc.tile(corpora["registered"], 700), 10000), 0xFFFFFFFF)
    want_rs, want_ok = dc.expected_rs(cases)
    blob, off, ln = dc.place(cases, seed, tight_end=tight)
    placed = off[ln != 0]
    assert set(int(o) % 16 for o in placed) == set(range(16))
    assert len(set(placed.tolist())) < len(placed)  # entries that share bytes
    if tight:
        assert int((off + np.minimum(ln, 72))[ln != 0].max()) == len(blob)
    assert (off[ln == 0] > len(blob)).all() and (ln == 0).any()
    rs, ok, mx = run_probe(H, blob, np.where(ln != 0, off, 0), ln)
    assert (ok == want_ok).all() and (rs == want_rs).all()
    assert (mx < np.minimum(ln, 72)).all()
    rs, ok, bad = run_dwords(H, blob, off, ln)
    assert (ok == want_ok).all(), [cases[i].name for i in np.nonzero(ok != want_ok)[0][:4]]
    assert (rs == want_rs).all()
    assert bad == 0


def check_fixed_length(H, arr):
    """the three readers against the oracle on the rows of arr (k, L): packed
    back to back, so every row but the last is followed by another encoding"""
    k, L = arr.shape
    blob = np.concatenate([np.ascontiguousarray(arr).reshape(-1), np.zeros(1, np.uint8)])
    raw = blob.tobytes()
    off = np.arange(k, dtype=np.uint64) * np.uint64(L)
    ln = np.full(k, L, np.uint32)
    want_rs, want_ok = np.zeros((k, 64), np.uint8), np.zeros(k, bool)
    to_rs = oder.to_rs
    for i in range(k):
        w = to_rs(raw[i * L:(i + 1) * L])
        if w is not None:
            want_rs[i], want_ok[i] = np.frombuffer(w, np.uint8), True
    rs, ok = run_ptr(H, blob, off, ln)
    assert (ok == want_ok).all(), [raw[i * L:(i + 1) * L].hex() for i in np.nonzero(ok != want_ok)[0][:4]]
    assert (rs == want_rs).all()
    rs, ok, mx = run_probe(H, blob, off, ln)
    assert (ok == want_ok).all() and (rs == want_rs).all() and (mx < min(L, 72)).all()
    rs, ok, bad = run_dwords(H, blob, off, ln)
    assert (ok == want_ok).all() and (rs == want_rs).all() and bad == 0
    return want_ok


def test_header_mutations(H, oracle_lib, corpora):
    """EVERY 1-byte and EVERY 2-byte mutation of the six header bytes (two
    tags and one length per level) of one valid 71-byte encoding: 6 x 256 and
    15 pairs x 65,536 = 983,040 encodings, each against the oracle behind all
    three readers.  Among them the pairs that keep the three lengths
    consistent with one another (45/20, 44/1f, ...), which then fail only at
    the integers' minimality or at the trailing bytes."""
    e = next(c.der for c in corpora["registered"] if c.valid_class and len(c.der) == 71)
    base = np.frombuffer(e, np.uint8)
    pos = dc._header_positions(e)
    assert len(pos) == 6 and len(set(pos)) == 6
    vals = np.arange(256, dtype=np.uint8)
    parsed = 0
    for p in pos:
        arr = np.tile(base, (256, 1))
        arr[:, p] = vals
        ok = check_fixed_length(H, arr)
        assert ok.sum() >= 1 and ok[e[p]]
        parsed += int(ok.sum())
    pairs = 0
    for p, q in itertools.combinations(pos, 2):
        arr = np.tile(base, (65536, 1))
        arr[:, p] = np.repeat(vals, 256)
        arr[:, q] = np.tile(vals, 256)
        ok = check_fixed_length(H, arr)
        assert ok[e[p] * 256 + e[q]]  # the untouched encoding is among them
        pairs += len(arr)
        parsed += int(ok.sum())
    assert pairs == 15 * 65536
    print("header mutations: %d encodings parsed of %d" % (parsed, pairs + 6 * 256))


def test_nothing_longer_than_72_bytes_parses(H):
    """the fact the kernel is built on, against the oracle (which keeps the
    long-form lengths): random inputs of 73..200 bytes, and long-form
    encodings crafted to be as plausible as the grammar allows"""
    rng = np.random.default_rng(72)
    ders = [rng.bytes(int(rng.integers(73, 201))) for _ in range(3000)]
    r32, s32 = b"\x7f" + rng.bytes(31), b"\x01" + rng.bytes(31)
    ints = [b"\x01", b"\x00\x80" + rng.bytes(31), r32, b"\x00" * 40 + r32, b"\x01" * 62, b"\x01" * 127, b"\x01" * 128,
            b"\x00" + b"\x80" * 128, b"\x7f" * 200]

    def tlvs(tag, content):
        out = [dc._tlv(tag, content)]
        n = len(content)
        for k in (1, 2, 3, 4, 5):  # every long form of the length, honest or not
            out.append(bytes([tag, 0x80 | k]) + (n % (1 << 8 * k)).to_bytes(k, "big") + content)
        return out

    for a in ints:
        for b in ints:
            for ra in tlvs(0x02, a):
                for sb in tlvs(0x02, b)[:2]:
                    for pad in (b"", b"\x00" * (128 - min(128, len(ra) + len(sb)))):
                        ders += tlvs(0x30, ra + sb + pad)
    ders += [d + b"\x00" for d in ders[3000::7]]
    want = [oder.to_rs(d) for d in ders]
    long_form = [len(d) > 72 or (len(d) > 1 and d[1] & 0x80) for d in ders]
    assert sum(long_form) > 5000 and sum(w is not None for w in want) > 0
    assert not any(w is not None and lf for w, lf in zip(want, long_form))
    ok = check_all_readers(H, ders)
    assert not ok[np.array(long_form)].any()
    # an integer's long form inside a short sequence, and parse() alone accepting what to_rs rejects
    d = dc._tlv(0x30, b"\x02\x81\x80" + b"\x01" * 128 + dc._tlv(0x02, b"\x01"))
    assert oder.parse(d) is not None and oder.to_rs(d) is None and not check_all_readers(H, [d]).any()


def test_stand_alone_program_under_sanitizers(oracle_lib, corpora, tmp_path):
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only): every corpus encoding in a heap block of exactly its
    size, so a read past the length it was given aborts the program."""
    exe = os.path.join(_CPP, "der_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DDER_MAIN", "-o", exe, _SRC], check=True)
    cases = dc.with_claim(corpora["registered"] + corpora["carried"], 10000)
    want_rs, want_ok = dc.expected_rs(cases)
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c, rs, ok in zip(cases, want_rs, want_ok):
            f.write(struct.pack("<II", len(c.der) if c.claim is None else c.claim, len(c.der)))
            f.write(c.der + bytes([int(ok)]) + rs.tobytes())
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "der: 0 mismatches over %d encodings, %d parsed" % (len(cases), int(want_ok.sum())) in p.stdout
