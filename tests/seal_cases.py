"""Inputs and expected bytes for the sealed wire forms (pbftv_seal_votes /
_replies / _preprepares): tests/test_wire_cpu.py (wire.h on the CPU) and
tests/test_gpu_seal.py.  Pure Python and NumPy.  Every expected byte comes from
oracle/gojson.py's *_signed forms; every expected signature from
tests/rfc6979_model.py over hashlib's SHA-256 of oracle/gojson.py's unsigned
form, DER through oracle/der.py's writer.

Message tuples are the ones pbftv.py's Columns classes take (msgpath_cases.py);
a pre-prepare case carries its client signature beside it: None is Go's nil
slice, b"" a non-nil empty one."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import rfc6979_model as model
import sign_cases as sc
from oracle import der as oder
from oracle import gojson

KINDS = ("vote", "reply", "preprepare")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
INTS = (0, 1, -1, 9, 10, -10, I64_MIN, I64_MAX, 1668519246, 10 ** 18, -(10 ** 18))
# every base64 residue and pad, the r||s length, every DER length the signer emits, one past them
SIG_LENS = (0, 1, 2, 3, 64, 68, 69, 70, 71, 72, 80)
NKEYS = 5
DISTINCT = 64  # messages per kind the model signs; longer batches tile them

# the string families tests/test_wire.py and the Go-JSON tests use: escapes,
# controls, HTML, U+2028/9, valid multi-byte, invalid and truncated UTF-8
PARTS = (b"x", b"Z", b"0", b"<", b">", b"&", b'"', b"\\", b"\t", b"\n", b"\r", b"\x00", b"\x01", b"\x1f", b"\x7f",
         b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xff", b"\xc2\xa2", b"\xe0\x9f\xbf", b"\xe0\xa0\x80", b"\xf0\x90\x80\x80",
         b"\xf4\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xef\xbf\xbd", b"\xe2\x82", b"\xc0\x80", b"\xed\xa0\x80", b"\x80")


def family_string(i: int, f: int) -> bytes:
    """String f of message i: empty every fifth time, else 1..7 parts cycled so
    that every part opens, ends and sits inside some string of every column."""
    k = 7 * i + 3 * f
    if k % 5 == 0:
        return b""
    return b"".join(PARTS[(k + j * (f + 1)) % len(PARTS)] for j in range(1 + k % 7))


def _int(i: int, f: int) -> int:
    return INTS[(i + 4 * f) % len(INTS)]


@functools.lru_cache(maxsize=None)
def distinct(kind: str):
    """DISTINCT (message, client signature) cases of a kind: the string families
    in every string column, the int64 extremes in every integer, and for
    pre-prepares has_request mixed, the client signature nil or of every length
    in SIG_LENS."""
    rng = np.random.default_rng(0x5EA1)
    out = []
    for i in range(DISTINCT):
        s = [family_string(i, f) for f in range(3)]
        if kind == "vote":
            out.append(((_int(i, 0), _int(i, 1), s[0], s[1], _int(i, 2)), None))
        elif kind == "reply":
            out.append(((_int(i, 0), _int(i, 1), s[0], s[1], s[2]), None))
        else:
            req = None if i % 4 == 3 else (_int(i, 2), s[1], s[2], _int(i, 3))
            rsig = None if i % 6 == 5 else rng.bytes(SIG_LENS[i % len(SIG_LENS)])
            out.append(((_int(i, 0), _int(i, 1), s[0], req), rsig))
    return tuple(out)


def preimage(kind: str, msg) -> bytes:
    return getattr(gojson, kind)(*msg)


def wire(kind: str, msg, req_sig, sig: bytes) -> bytes:
    if kind == "preprepare":
        return gojson.preprepare_signed(*msg, req_sig, sig)
    return getattr(gojson, kind + "_signed")(*msg, sig)


def key_of(i: int) -> int:
    return (3 * i + i // 7) % NKEYS


@functools.lru_cache(maxsize=None)
def signed(kind: str):
    """Per distinct case under key key_of(i): (digest, r||s, DER), the model's."""
    ds = sc.keypool(NKEYS)
    out = []
    for i, (msg, _) in enumerate(distinct(kind)):
        dg = hashlib.sha256(preimage(kind, msg)).digest()
        rs = model.sign_bytes(dg, ds[key_of(i)])
        out.append((dg, rs, sc.der_expected(rs)))
    return tuple(out)


def batch(kind: str, n: int):
    """(messages, client signatures, key indices) of n messages: the distinct
    cases tiled."""
    d = distinct(kind)
    msgs = [d[i % DISTINCT][0] for i in range(n)]
    rsigs = [d[i % DISTINCT][1] for i in range(n)]
    kidx = np.array([key_of(i % DISTINCT) for i in range(n)], np.uint32)
    return msgs, rsigs, kidx


def expected(kind: str, n: int, der: bool):
    """(wire forms, digests (n, 32)) of batch(kind, n)."""
    d, s = distinct(kind), signed(kind)
    wires = [wire(kind, d[i % DISTINCT][0], d[i % DISTINCT][1], s[i % DISTINCT][2 if der else 1]) for i in range(n)]
    digests = np.frombuffer(b"".join(s[i % DISTINCT][0] for i in range(n)), np.uint8).reshape(n, 32)
    return wires, digests


def columns(kind: str, msgs):
    from simple_pbft_amd.pbftv import PrePrepareColumns, ReplyColumns, VoteColumns
    return {"vote": VoteColumns, "reply": ReplyColumns, "preprepare": PrePrepareColumns}[kind](msgs)


def check_layout(sealed, wires):
    """blob, offsets, lengths and total against the expected wire forms (b""
    for an unsigned row)."""
    blob, off, ln, _, ok = sealed
    want_len = np.array([len(w) for w in wires], np.uint64)
    want_off = np.concatenate([[0], np.cumsum(want_len)[:-1]]).astype(np.uint64) if len(wires) else want_len
    assert ln.tolist() == want_len.tolist()
    assert off.tolist() == want_off.tolist()
    assert len(blob) == int(want_len.sum())
    assert ok.tolist() == [len(w) > 0 for w in wires]
    got = blob.tobytes()
    if got != b"".join(wires):
        for i, w in enumerate(wires):
            assert sealed[i] == w, (i, sealed[i], w)
        raise AssertionError("blob differs outside the messages")


def rs_to_der(rs_row) -> bytes:
    return oder.encode(int.from_bytes(bytes(rs_row[:32]), "big"), int.from_bytes(bytes(rs_row[32:]), "big"))
