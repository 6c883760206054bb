"""Signatures as ASN.1 DER for tests/test_der_cpu.py, tests/test_gpu_der.py and
tests/test_gpu_flush_der.py: the corpus, its placement in a string column, and
the expected values.  Every expectation comes from oracle/der.py (``to_rs``;
None means a 0 bit) and the oracle's verify, never from the code under test.

A corpus is a list of Case; ``Case.full`` are the bytes put into the blob and
``Case.der`` (a prefix of them) the encoding the entry names, so a truncated
encoding is followed in memory by exactly the bytes that would complete it: a
parser that reads past the length it was given accepts it, and the oracle
does not."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass

import numpy as np

import varbase_cases as vc
from conftest import GOLDEN, fixture_arrays
from oracle import der as oder

N = vc.N
HEADER_VALUES = (0x00, 0x02, 0x30, 0x31, 0x7F, 0x80, 0x81, 0x82, 0xFF)

_cache: dict = {}


@dataclass
class Case:
    name: str
    der: bytes            # the encoding: the first len(der) bytes of `full`
    full: bytes           # what lies in memory from the encoding's first byte on
    row: int              # the base vector (hash and key) it is checked under
    valid_class: bool     # one of the "valid signature" classes (most of them need only parse)
    claim: int | None = None   # lengths[i] where it is not len(der)
    far: bool = False     # a length-0 entry whose offset lies far outside the blob


def golden_registered():
    """keys (k, 64), hashes, r||s, key_idx of the golden ECDSA vectors"""
    with open(os.path.join(GOLDEN, "ecdsa.json")) as f:
        fx = json.load(f)
    keys, hashes, sigs, kidx, _ = fixture_arrays(fx)
    return keys, hashes, sigs, kidx


def _rs_ints(rs):
    b = bytes(rs)
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")


def _tlv(tag: int, content: bytes, length: bytes | None = None) -> bytes:
    return bytes([tag]) + (oder._len(len(content)) if length is None else length) + content


def raw(r: bytes, s: bytes) -> bytes:
    """SEQUENCE of two INTEGERs with the given content bytes, lengths minimal"""
    return _tlv(0x30, _tlv(0x02, r) + _tlv(0x02, s))


def _header_positions(enc: bytes):
    lr = enc[3]
    return (0, 1, 2, 3, 4 + lr, 5 + lr)


def build(sigs: np.ndarray, accepted: np.ndarray) -> list:
    """The corpus over base vectors with r||s rows `sigs`, of which `accepted`
    are the ones the oracle verifies: valid and rejected cases interleaved,
    a valid one first, the valid classes cycled so that every prefix of the
    list holds at least as many valid-class cases as rejected ones."""
    valid, rejected = [], []
    enc = [oder.encode(*_rs_ints(row)) for row in sigs]
    assert all(oder.to_rs(e) == bytes(sigs[i]) for i, e in enumerate(enc))
    for i, e in enumerate(enc):
        valid.append(Case("vector %d" % i, e, e, i, True))
    ok_rows = np.nonzero(accepted)[0]
    base = int(ok_rows[0])
    r0, s0 = _rs_ints(sigs[base])
    # integers of every minimal length 1..33, for r and for s
    for nbytes in range(1, 34):
        v = (1 << (8 * nbytes - 1)) - 1 if nbytes < 33 else (1 << 255) | 1  # 33: the 00 pad and 32 bytes
        e_r, e_s = oder.encode(v, s0), oder.encode(r0, v)
        assert e_r[3] == nbytes and e_s[5 + e_s[3]] == nbytes
        assert oder.to_rs(e_r) is not None and oder.to_rs(e_s) is not None
        valid.append(Case("r of %d bytes" % nbytes, e_r, e_r, base, True))
        valid.append(Case("s of %d bytes" % nbytes, e_s, e_s, base, True))
    for name, r, s in (("r = 0", 0, s0), ("s = 0", r0, 0), ("r = n", N, s0), ("s = n", r0, N),
                       ("r = 2^256 - 1", (1 << 256) - 1, s0), ("s = n + 1", r0, N + 1)):
        e = oder.encode(r, s)
        assert oder.to_rs(e) is not None
        valid.append(Case(name, e, e, base, True))

    # rejected encodings of a valid 70-, 71- and 72-byte encoding
    by_len = {}
    for i in ok_rows:
        by_len.setdefault(len(enc[i]), int(i))
    assert {70, 71, 72} <= set(by_len), sorted(by_len)
    for L in (70, 71, 72):
        row, e = by_len[L], enc[by_len[L]]
        rj = lambda name, d, full=None, **kw: rejected.append(  # noqa: E731
            Case("%d-byte: %s" % (L, name), d, d if full is None else full, row, False, **kw))
        for pos in _header_positions(e):
            for v in HEADER_VALUES:
                if e[pos] != v:
                    rj("header byte %d = %02x" % (pos, v), e[:pos] + bytes([v]) + e[pos + 1:])
        for cut in (1, 2, 3, 4, 5, 6):
            rj("truncated by %d" % cut, e[:-cut], e)
        for keep in (0, 1, 2):
            rj("truncated to %d" % keep, e[:keep], e, far=keep == 0)
        rj("trailing byte inside the sequence", bytes([0x30, e[1] + 1]) + e[2:] + b"\x00")
        rj("trailing byte after the sequence", e + b"\x00")
        body = e[2:]
        rj("sequence length 81 %02x" % len(body), b"\x30\x81" + bytes([len(body)]) + body)
        rj("sequence length 82 00 %02x" % len(body), b"\x30\x82\x00" + bytes([len(body)]) + body)
        rj("sequence length 84", b"\x30\x84\x00\x00\x00" + bytes([len(body)]) + body)
        rj("sequence length 85", b"\x30\x85\x00\x00\x00\x00" + bytes([len(body)]) + body)
        big = _tlv(0x02, b"\x01" * 62) + _tlv(0x02, b"\x01" * 62)  # 128 content bytes, honestly long-form
        assert len(big) == 128
        rj("sequence length 81 80", b"\x30\x81\x80" + big)
        rj("sequence length 81 80 around the valid integers", b"\x30\x81\x80" + body + b"\x00" * (128 - len(body)))
        rb, sb = e[4:4 + e[3]], e[6 + e[3]:]
        rj("r length 81 %02x" % len(rb), _tlv(0x30, _tlv(0x02, rb, b"\x81" + bytes([len(rb)])) + _tlv(0x02, sb)))
        rj("r of 128 bytes", _tlv(0x30, _tlv(0x02, b"\x01" * 128) + _tlv(0x02, sb)))
        sv = sb.lstrip(b"\x00") or b"\x01"
        for name, rr in (("00 00 ..", b"\x00\x00" + sv[:30]), ("00 7f ..", b"\x00\x7f" + sv[:30]),
                         ("ff 80 ..", b"\xff\x80" + sv[:30]), ("ff ff ..", b"\xff\xff" + sv[:30]),
                         ("negative", b"\x80" + sv[:31]), ("34 bytes with 00", b"\x00\x80" + sv[:32].rjust(32, b"\x01")),
                         ("34 bytes", b"\x01\x80" + sv[:32].rjust(32, b"\x01")),
                         ("33 bytes without 00", b"\x01" + sv[:32].rjust(32, b"\x01")), ("length 0", b"")):
            rj("r " + name, raw(rr, sb))
            rj("s " + name, raw(rb, rr))
        rj("length 0, offset far outside", b"", far=True)
    assert all(oder.to_rs(c.der) is None for c in rejected), [c.name for c in rejected if oder.to_rs(c.der)][:4]
    out = []
    for k, c in enumerate(rejected):
        out += [valid[k % len(valid)], c]
    for c in valid[len(rejected) % len(valid):] if len(rejected) < len(valid) else []:
        out.append(c)
    return out


def want_rs(c: Case):
    """oracle/der.to_rs of what entry c names.  A claimed length beyond the
    real bytes cannot be materialised: by the 72-byte fact (proved against the
    oracle in tests/test_der_cpu.py) nothing longer than 72 bytes parses."""
    if c.claim is not None and c.claim != len(c.der):
        assert c.claim > 72
        return None
    return oder.to_rs(c.der)


def expected_rs(cases) -> tuple:
    """(n x 64 r||s with zero rows where to_rs is None, parsed bool[n])"""
    rs = np.zeros((len(cases), 64), np.uint8)
    ok = np.zeros(len(cases), bool)
    for i, c in enumerate(cases):
        w = want_rs(c)
        if w is not None:
            rs[i] = np.frombuffer(w, np.uint8)
            ok[i] = True
    return rs, ok


def tile(corpus, n):
    return [corpus[i % len(corpus)] for i in range(n)]


def place(cases, seed: int, tight_end: bool = True, min_bytes: int = 0):
    """blob, offsets (u64), lengths (u32): the entries in shuffled memory order,
    random non-zero filler before and between them, their first bytes walking
    through every offset modulo 16, equal `full` bytes placed once and shared
    every second time they recur, and (tight_end) the last encoding ending on
    the last byte of the blob.  min_bytes: filler appended up to that size
    (for a claimed length that must stay inside the blob)."""
    rng = np.random.default_rng(seed)
    n = len(cases)
    off = np.zeros(n, np.uint64)
    ln = np.zeros(n, np.uint32)
    blob = bytearray(rng.integers(1, 256, 5, dtype=np.uint8).tobytes())
    seen: dict = {}
    order = rng.permutation(n)
    if tight_end:  # an entry that reaches the end of its bytes goes last in memory: one with a claimed length first
        full = [int(j) for j in order[::-1] if len(cases[j].der) == len(cases[j].full) and cases[j].der]
        k = next((j for j in full if cases[j].claim is not None), full[0])
        order = np.array([j for j in order if j != k] + [k])
    for step, i in enumerate(order):
        c = cases[int(i)]
        ln[i] = len(c.der) if c.claim is None else c.claim
        if c.far or not c.full:
            off[i] = (1 << 40) + 977 * int(i)
            continue
        hit = seen.get(c.full)
        if hit is not None and hit[1] % 2 == 0 and not (tight_end and step == n - 1):
            off[i] = hit[0]
            seen[c.full] = (hit[0], hit[1] + 1)
            continue
        pad = (step % 16 - len(blob)) % 16
        blob += rng.integers(1, 256, pad, dtype=np.uint8).tobytes()
        off[i] = len(blob)
        blob += c.full
        seen[c.full] = (int(off[i]), 0 if hit is None else hit[1] + 1)
    if len(blob) < min_bytes:
        blob += rng.integers(1, 256, min_bytes - len(blob), dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(blob), np.uint8).copy(), off, ln


def registered_corpus(oracle_lib):
    """(keys, hashes, key_idx, corpus): the golden vectors as base rows"""
    if "reg" not in _cache:
        keys, hashes, sigs, kidx = golden_registered()
        acc = vc.oracle_expect_keyed(oracle_lib, hashes, sigs, keys, np.minimum(kidx, len(keys) - 1)) & (kidx < len(keys))
        _cache["reg"] = (keys, hashes, kidx, build(sigs, acc))
    return _cache["reg"]


def carried_corpus(oracle_lib):
    """(hashes, pubs, corpus): varbase_cases.all_vectors as base rows"""
    if "car" not in _cache:
        h, s, p, want = vc.all_vectors(oracle_lib)
        _cache["car"] = (h, p, build(s, want))
    return _cache["car"]


def _tiled(corpus, want, n, claim):
    """corpus rows, cases, r||s, parsed, bits for the corpus tiled to n; with
    `claim` (and n > 1) the last entry is a valid 72-byte encoding whose
    length is claimed as `claim`: nothing that long parses, so a 0 bit"""
    rows, rs, ok, bits = want
    idx = np.arange(n) % len(corpus)
    cases, rows, rs, ok, bits = tile(corpus, n), rows[idx].copy(), rs[idx].copy(), ok[idx].copy(), bits[idx].copy()
    if claim is not None and n > 1:
        cases[-1] = with_claim(corpus, claim)[-1]
        rows[-1], rs[-1], ok[-1], bits[-1] = cases[-1].row, 0, False, False
    return rows, cases, np.ascontiguousarray(rs), ok, bits


def registered_batch(oracle_lib, n, claim=None):
    """hashes, key_idx, cases, r||s, parsed, expected verify bits -- the corpus tiled to n"""
    keys, hashes, kidx, corpus = registered_corpus(oracle_lib)
    if "reg_want" not in _cache:
        rows = np.array([c.row for c in corpus])
        rs, ok = expected_rs(corpus)
        k = kidx[rows]
        inside = k < len(keys)
        bits = vc.oracle_expect_keyed(oracle_lib, hashes[rows], rs, keys, np.where(inside, k, 0)) & inside & ok
        _cache["reg_want"] = (rows, rs, ok, bits)
    rows, cases, rs, ok, bits = _tiled(corpus, _cache["reg_want"], n, claim)
    return np.ascontiguousarray(hashes[rows]), np.ascontiguousarray(kidx[rows]), cases, rs, ok, bits


def carried_batch(oracle_lib, n, claim=None):
    """hashes, pubs (X||Y), cases, r||s, parsed, expected verify bits under X||Y keys"""
    hashes, pubs, corpus = carried_corpus(oracle_lib)
    if "car_want" not in _cache:
        rows = np.array([c.row for c in corpus])
        rs, ok = expected_rs(corpus)
        bits = vc.oracle_expect(oracle_lib, hashes[rows], rs, pubs[rows]) & ok
        _cache["car_want"] = (rows, rs, ok, bits)
    rows, cases, rs, ok, bits = _tiled(corpus, _cache["car_want"], n, claim)
    return np.ascontiguousarray(hashes[rows]), np.ascontiguousarray(pubs[rows]), cases, rs, ok, bits


def with_claim(cases, claim: int):
    """the cases with one more entry: a valid 72-byte encoding whose length is
    claimed as `claim` (its row's hash and key must be appended by the caller
    from .row)"""
    c = next(c for c in cases if c.valid_class and len(c.der) == 72 and c.name.startswith("vector"))
    return cases + [Case("72 bytes claimed as %d" % claim, c.der, c.full, c.row, False, claim=claim)]


def check_corpus(corpus, bits):
    """the corpus holds accepted and rejected signatures, and the valid classes
    are at least half of it and of every prefix"""
    assert bits.any() and not bits.all()
    v = np.array([c.valid_class for c in corpus])
    assert (np.cumsum(v) * 2 >= np.arange(1, len(v) + 1)).all()
