"""Chosen inputs for the message path -- the lane-per-message Go-JSON encoder
(gojson_kernels.hip) feeding the lane-per-message SHA-256 (sha256_kernels.hip)
-- for tests/test_msgpath_cases.py (CPU), tests/test_gpu_sha_seams.py and
tests/test_gpu_gojson_seams.py.  Pure Python and NumPy: nothing here touches a
GPU, and every expected value the tests use comes from hashlib and
oracle/gojson.py.

Message tuples are the ones pbftv.py's Columns classes take:
  request     (timestamp, clientID, operation, sequenceID)
  vote        (viewID, sequenceID, digest, nodeID, msgType)
  reply       (viewID, timestamp, clientID, nodeID, result)
  preprepare  (viewID, sequenceID, digest, request | None)
"""
from __future__ import annotations

import copy
import hashlib

import numpy as np

from oracle import gojson

KINDS = ("request", "vote", "reply", "preprepare")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

# ------------------------------------------------------------------ SHA-256 sweep
SHA_RESIDUES = 128            # k_sha256_ring: the message's byte position in its 128-B line
SHA_DENSE_MAX = 704           # 11 full blocks: start-up, two ring periods of 4 blocks, every tail at every phase
SHA_LONG_LENGTHS = (4095, 4096, 4097, 8191, 65463, 65464, 65535, 65536, 65537, 200001)  # 65464: bucket_of clamps
SHA_LONG_RESIDUES = (0, 1, 3, 4, 63, 64, 124, 127)
SHA_SWEEP_N = SHA_RESIDUES * (SHA_DENSE_MAX + 1) + len(SHA_LONG_LENGTHS) * len(SHA_LONG_RESIDUES)  # 90,320


def sha_sweep_max_bytes() -> int:
    """An upper bound of len(sha_sweep(b)[0]) for every b: each message is
    preceded by a gap of at most 127 bytes."""
    dense = SHA_RESIDUES * sum(range(SHA_DENSE_MAX + 1))
    long_ = len(SHA_LONG_RESIDUES) * sum(SHA_LONG_LENGTHS)
    return dense + long_ + 127 * SHA_SWEEP_N


def sha_sweep(base_residue: int):
    """(blob, offsets, lengths): one message for every residue 0..127 of
    (base_residue + offset) % 128 and every length 0..704, then 80 long ones;
    each at the lowest free position with its residue.  The blob, gaps
    included, is seeded random bytes."""
    assert 0 <= base_residue < SHA_RESIDUES
    pairs = [(r, ln) for ln in range(SHA_DENSE_MAX + 1) for r in range(SHA_RESIDUES)]
    pairs += [(r, ln) for ln in SHA_LONG_LENGTHS for r in SHA_LONG_RESIDUES]
    n = len(pairs)
    offsets = np.zeros(n, np.uint64)
    lengths = np.zeros(n, np.uint32)
    pos = 0
    for i, (r, ln) in enumerate(pairs):
        pos += (r - base_residue - pos) % SHA_RESIDUES
        offsets[i] = pos
        lengths[i] = ln
        pos += ln
    blob = np.frombuffer(np.random.default_rng(0x5EA5).bytes(pos), np.uint8)
    assert n == SHA_SWEEP_N and n % 32 and n % 64 and n % 256
    seen = set(zip(((offsets + np.uint64(base_residue)) % np.uint64(SHA_RESIDUES)).tolist(), lengths.tolist()))
    assert all((r, ln) in seen for r in range(SHA_RESIDUES) for ln in range(SHA_DENSE_MAX + 1))
    assert len(blob) <= sha_sweep_max_bytes()
    return blob, offsets, lengths


def sha_expected(blob, offsets, lengths) -> np.ndarray:
    """hashlib's digest of every message, n x 32."""
    mv = memoryview(np.ascontiguousarray(blob))
    out = bytearray()
    for o, ln in zip(offsets.tolist(), lengths.tolist()):
        out += hashlib.sha256(mv[o:o + ln]).digest()
    return np.frombuffer(bytes(out), np.uint8).reshape(len(lengths), 32)


def sha_blocks(lengths) -> np.ndarray:
    """bucket_of (sha256_kernels.hip): compression calls per message, clamped at 1023."""
    return np.minimum((np.asarray(lengths).astype(np.int64) + 8) // 64 + 1, 1023)


# ------------------------------------------------------------------ Go-JSON bounds
SIXFOLD = (0x00, 0x1F, 0x3C, 0x3E, 0x26, 0x80, 0xC0, 0xF5, 0xFF)  # each byte encodes to six
BOUND_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 43, 64)
BOUND_N = 257  # crosses a 256-lane block
BOUND_BASE = {"request": 97, "vote": 120, "reply": 102, "preprepare": 188}  # encoded length at sum L = 0


def _sixfold(length: int, start: int) -> bytes:
    return bytes(SIXFOLD[(start + k) % len(SIXFOLD)] for k in range(length))


def _field_lengths(j: int, fields: int) -> list[int]:
    """Lengths of message j's string fields: the first two run through every
    pair of BOUND_LENGTHS, a third is offset from them."""
    q = len(BOUND_LENGTHS)
    idx = [j % q, (j // q) % q, (2 * j + 5) % q]
    return [BOUND_LENGTHS[idx[f]] for f in range(fields)]


def string_fields(kind: str, msg) -> list[bytes]:
    """The byte-string fields of a message tuple (a nil request has none)."""
    if kind == "request":
        return [msg[1], msg[2]]
    if kind == "vote":
        return [msg[2], msg[3]]
    if kind == "reply":
        return [msg[2], msg[3], msg[4]]
    return [msg[2]] + ([msg[3][1], msg[3][2]] if msg[3] is not None else [])


def _message(kind: str, ints, strs, with_request: bool = True):
    """A message tuple from its integers and strings in struct order."""
    if kind == "request":
        return (ints[0], strs[0], strs[1], ints[1])
    if kind == "vote":
        return (ints[0], ints[1], strs[0], strs[1], ints[2])
    if kind == "reply":
        return (ints[0], ints[1], strs[0], strs[1], strs[2])
    req = (ints[2], strs[1], strs[2], ints[3]) if with_request else None
    return (ints[0], ints[1], strs[0], req)


_N_INTS = {"request": 2, "vote": 3, "reply": 2, "preprepare": 4}
_N_STRS = {"request": 2, "vote": 2, "reply": 3, "preprepare": 3}


def gojson_bound_cases(kind: str):
    """(messages, sorts): 257 messages, sorts[i] in {"bound", "minimal",
    "plain"} interleaved.  A "bound" message has every integer -2^63 and every
    string made of bytes that encode sixfold, so it fills its slot
    (request_bound / vote_bound / reply_bound) to the last byte, or to the
    last but one for a pre-prepare; about one pre-prepare in five is nil."""
    assert kind in KINDS
    ni, ns = _N_INTS[kind], _N_STRS[kind]
    msgs, sorts = [], []
    for i in range(BOUND_N):
        sort = ("bound", "minimal", "plain")[i % 3]
        j = i // 3
        lens = _field_lengths(j, ns)
        if sort == "bound":
            ints, strs = [I64_MIN] * ni, [_sixfold(ln, j + 3 * f) for f, ln in enumerate(lens)]
        elif sort == "minimal":
            ints, strs = [0] * ni, [b""] * ns
        else:
            ints, strs = [1 + 977 * i + f for f in range(ni)], [b"x" * ln for ln in lens]
        msgs.append(_message(kind, ints, strs, with_request=i % 5 != 4))
        sorts.append(sort)
    return msgs, sorts


def encode(kind: str, msg) -> bytes:
    """oracle/gojson.py's encoding of a message tuple."""
    return getattr(gojson, kind)(*msg)


# ------------------------------------------------------------------ UTF-8 edges
# truncated prefix -> the bytes that would complete it (e2 | 80 a8 is U+2028)
UTF8_PREFIXES = ((b"\xc2", b"\xa2"), (b"\xe2", b"\x80\xa8"), (b"\xe2\x80", b"\xa8"), (b"\xe0\xa0", b"\x80"),
                 (b"\xed\x9f", b"\xbf"), (b"\xf0", b"\x90\x80\x80"), (b"\xf0\x90", b"\x80\x80"),
                 (b"\xf0\x90\x80", b"\x80"), (b"\xf4\x8f\xbf", b"\xbf"))
UTF8_EXACT = (b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xef\xbf\xbd")


def utf8_edge_strings() -> list[list[bytes]]:
    """Nine columns of strings, one per truncated prefix.  In each, for every
    prefix p with completion c, adjacent strings  "ab" + p | c + "cd"  and
    p | c  (packed in message order, the second begins where the first's
    sequence would go on), the three exact strings, and the column's own
    prefix as the last string of its blob."""
    body = []
    for p, c in UTF8_PREFIXES:
        body += [b"ab" + p, c + b"cd", p, c]
    body += list(UTF8_EXACT)
    return [body + [p] for p, _ in UTF8_PREFIXES]


def utf8_messages(kind: str, col: list[bytes]):
    """One message per string of col, the string in every string field."""
    return [_message(kind, [i, -i, 3 * i, 7][:_N_INTS[kind]], [s] * _N_STRS[kind], with_request=i % 6 != 5)
            for i, s in enumerate(col)]


# ------------------------------------------------------------------ long strings
LONG_LENGTHS = (1023, 1024, 4096, 65535, 65536, 70001)
LONG_ZERO_OPERATION = 65536  # one operation of this many 00 bytes: a 393 KB preimage


def _cycled(length: int, start: int) -> bytes:
    from test_gpu_messages import ALPHABET  # every encodeState.string branch
    out, k = bytearray(), start
    while len(out) < length:
        out += ALPHABET[k % len(ALPHABET)]
        k += 1
    return bytes(out[:length])


def long_string_cases() -> dict:
    """kind -> about 70 messages: short ones, and among them one with a long
    operation (request, pre-prepare), result (reply) or digest (vote,
    pre-prepare) per LONG_LENGTHS, plus one operation of 65536 x 00."""
    rng = np.random.default_rng(0x10E6)
    out = {}
    for kind in KINDS:
        ni, ns = _N_INTS[kind], _N_STRS[kind]
        msgs = []
        for i in range(64):
            ints = [int(x) for x in rng.integers(-10 ** 6, 10 ** 12, ni)]
            strs = [_cycled(int(rng.integers(0, 24)), int(rng.integers(0, 30))) for _ in range(ns)]
            msgs.append(_message(kind, ints, strs, with_request=i % 7 != 3))
        longs = []
        where = {"request": [1], "vote": [0], "reply": [2], "preprepare": [0, 2]}[kind]
        for f in where:
            for k, ln in enumerate(LONG_LENGTHS):
                strs = [b"n%d" % k] * ns
                strs[f] = _cycled(ln, k)
                longs.append(_message(kind, [k, -k, 5, 6][:ni], strs))
        if kind in ("request", "preprepare"):
            strs = [b"c"] * ns
            strs[-1] = bytes(LONG_ZERO_OPERATION)
            longs.append(_message(kind, [1, 2, 3, 4][:ni], strs))
        for k, m in enumerate(longs):  # spread among the short ones, the first at lane 0
            msgs.insert(min(len(msgs), k * 5), m)
        out[kind] = msgs
    return out


# ------------------------------------------------------------------ column layouts
LAYOUTS = ("reversed", "interned", "gapped", "empties")


def string_columns(cols) -> list[str]:
    """Names of a Columns object's (blob, off, len) attributes."""
    return [k for k, v in vars(cols).items() if isinstance(v, tuple) and len(v) == 3]


def column_strings(col) -> list[bytes]:
    blob, off, ln = col
    b = blob.tobytes()
    return [b[int(o):int(o) + int(n)] if n else b"" for o, n in zip(off, ln)]


def _layout(strs: list[bytes], how: str, rng):
    n = len(strs)
    off = np.zeros(n, np.uint64)
    ln = np.array([len(s) for s in strs], np.uint32)
    buf = bytearray()
    if how == "reversed":  # the last message's string first
        for i in reversed(range(n)):
            off[i] = len(buf)
            buf += strs[i]
    elif how == "interned":  # equal strings stored once
        at = {}
        for i, s in enumerate(strs):
            if s not in at:
                at[s] = len(buf)
                buf += s
            off[i] = at[s]
    elif how == "gapped":  # junk before the first string and between strings
        buf += rng.bytes(1000)
        for i, s in enumerate(strs):
            off[i] = len(buf)
            buf += s + rng.bytes(1 + i % 9)
    elif how == "empties":  # packed; an empty string's offset is inside the blob, or one past its end
        for i, s in enumerate(strs):
            off[i] = len(buf)
            buf += s
        k = 0
        for i, s in enumerate(strs):
            if not s:
                off[i] = len(buf) if k % 2 else len(buf) // 2
                k += 1
    else:
        raise ValueError(how)
    blob = np.frombuffer(bytes(buf), np.uint8) if buf else np.zeros(1, np.uint8)
    return np.ascontiguousarray(blob), off, ln


def relayout(cols, how: str):
    """A copy of a packed RequestColumns / VoteColumns / ReplyColumns /
    PrePrepareColumns whose string columns hold the same strings laid out
    differently (LAYOUTS)."""
    rng = np.random.default_rng(0x1A70)
    out = copy.copy(cols)
    for name in string_columns(cols):
        setattr(out, name, _layout(column_strings(getattr(cols, name)), how, rng))
    return out


def layout_batch(kind: str, n: int):
    """n messages for the layout tests: digests drawn from 3 values and node /
    client ids from 4 (so interning bites), operations and results distinct,
    every seventh string of a column empty.  Four pre-prepares in seven embed
    one of three requests and carry its digest (verifyMsg can pass); the
    others carry one of the three digests above."""
    digs = [hashlib.sha256(b"layout %d" % k).hexdigest().encode() for k in range(3)]
    ids = [b"node%d" % k for k in range(4)]
    reqs = [(k, ids[k] + b"<c>", b"op %d" % k, 100 + k) for k in range(3)]
    req_digs = [hashlib.sha256(gojson.request(*r)).hexdigest().encode() for r in reqs]
    msgs = []
    for i in range(n):
        e = i % 7 == 6
        d = b"" if e else digs[(i * 5) % 3]
        node = b"" if i % 7 == 5 else ids[(i * 3) % 4]
        cid = b"" if i % 7 == 4 else ids[(i * 7 + 1) % 4] + b"<c>"
        text = b"" if i % 7 == 3 else b"op\xe2\x80\xa8 %d \xff" % i
        if kind == "request":
            msgs.append((i, cid, text, -i))
        elif kind == "vote":
            msgs.append((i % 11, i, d, node, i % 2))
        elif kind == "reply":
            msgs.append((i % 11, 10 ** 15 + i, cid, node, text))
        elif i % 7 in (0, 1, 2, 5) and i % 6 != 1:
            msgs.append((i % 11, i, req_digs[(i * 5) % 3], reqs[(i * 5) % 3]))
        else:
            msgs.append((i % 11, i, d, None if i % 6 == 1 else (i, cid, text, i)))
    return msgs


# ------------------------------------------------------------------ verifyMsg edges
def _ints(*vals):
    return sorted({v for v in vals if I64_MIN <= v <= I64_MAX})


def verify_msg_edges(right_hex):
    """Rows (state view, state last_seq, view, seq, digest bytes, state index)
    for State.verifyMsg (pbft_impl.go:176-202).  right_hex(j) is the lowercase
    hex digest that row j's state expects.  The state table the rows speak of
    has one state per row, k = len(rows): row j is addressed to state j, except
    the last rows, which repeat passing rows with the index k or 0xFFFFFFFF
    (out of range: the bit is 0).  Rows 0 and k - 1 pass."""
    views = [(7, 7), (7, 8), (7, 6), (7, I64_MIN), (7, I64_MAX), (I64_MIN, I64_MIN), (I64_MAX, I64_MAX),
             (I64_MIN, I64_MAX), (I64_MAX, I64_MIN)]
    core = [(7, -1, 7, 0)]  # a passing row first
    for seq in (I64_MIN, -1, 0, I64_MAX):
        for last in _ints(-1, seq - 1, seq, seq + 1, I64_MIN, I64_MAX):
            for sv, view in views:
                core.append((sv, last, view, seq))
    rows = [(sv, last, view, seq, None) for sv, last, view, seq in core]

    def variants(h: bytes):
        first = (b"0" if h[:1] != b"0" else b"1") + h[1:]
        last = h[:-1] + (b"f" if h[-1:] != b"f" else b"e")
        out = [b"", h[:63], h, h + b"0", h.upper(), first, last]
        for pos in (0, 31, 63):
            for ch in (b"/", b":", b"`", b"g", b"G", b"@"):
                out.append(h[:pos] + ch + h[pos + 1:])
        return out

    n_var = len(variants(b"a" * 64))
    for sv, last, view, seq in ((7, -1, 7, 0), (I64_MIN, I64_MIN, I64_MIN, I64_MAX), (I64_MAX, I64_MAX - 1, I64_MAX,
                                                                                       I64_MAX)):
        rows += [(sv, last, view, seq, v) for v in range(n_var)]
    passing = [(7, -1, 7, 5, None), (7, 4, 7, 5, None)]
    n_oob = 4
    k = len(rows) + n_oob + 1
    out = []
    for j, (sv, last, view, seq, v) in enumerate(rows):
        h = right_hex(j)
        out.append((sv, last, view, seq, h if v is None else variants(h)[v], j))
    for t, idx in enumerate((k, 0xFFFFFFFF, k, 0xFFFFFFFF)):
        sv, last, view, seq, _ = passing[t % 2]
        out.append((sv, last, view, seq, right_hex(len(out)), idx))
    sv, last, view, seq, _ = passing[1]
    out.append((sv, last, view, seq, right_hex(len(out)), len(out)))  # state k - 1, passing
    assert len(out) == k and out[-1][5] == k - 1 and out[0][5] == 0
    return out
