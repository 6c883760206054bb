"""The case builders of tests/msgpath_cases.py checked without a GPU: the
SHA-256 sweep covers what it claims, the at-bound messages sit at the encoder's
bounds by the oracle (oracle/gojson.py) and by the host encoder alone, every
layout holds the packed strings, and the UTF-8 edges encode the same way in
the oracle and the host encoder."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import msgpath_cases as mc
from conftest import ROOT
from oracle import gojson


@pytest.fixture(scope="module")
def pb():
    from simple_pbft_amd import pbftv
    if not os.path.exists(pbftv.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "simple_pbft_amd"), "-j8"], check=True)
    return pbftv


def host_length(pb, kind, msg) -> int:
    """The host encoder's length of a message, asked with cap = 0."""
    L = pb.lib()
    if kind == "request":
        ts, cid, op, seq = msg
        return L.pbftv_gojson_request(ts, cid, len(cid), op, len(op), seq, None, 0)
    if kind == "vote":
        view, seq, dg, node, mt = msg
        return L.pbftv_gojson_vote(view, seq, dg, len(dg), node, len(node), mt, None, 0)
    if kind == "reply":
        view, ts, cid, node, res = msg
        return L.pbftv_gojson_reply(view, ts, cid, len(cid), node, len(node), res, len(res), None, 0)
    view, seq, dg, req = msg
    if req is None:
        return L.pbftv_gojson_preprepare(view, seq, dg, len(dg), 0, 0, b"", 0, b"", 0, 0, None, 0)
    ts, cid, op, rseq = req
    return L.pbftv_gojson_preprepare(view, seq, dg, len(dg), 1, ts, cid, len(cid), op, len(op), rseq, None, 0)


def host_encode(pb, kind, msg) -> bytes:
    return getattr(pb, "gojson_" + kind)(*msg)


def slot_bound(kind, msg) -> int:
    """gojson_enc.h's request_bound / vote_bound / reply_bound / preprepare_bound."""
    six = 6 * sum(len(s) for s in mc.string_fields(kind, msg))
    return {"request": 97, "vote": 120, "reply": 102, "preprepare": 92 + 97}[kind] + six  # (nil request: lengths 0)


@pytest.mark.parametrize("base", [0, 1, 64, 127])
def test_sha_sweep_covers_every_residue_and_length(base):
    blob, off, ln = mc.sha_sweep(base)
    assert len(ln) == mc.SHA_SWEEP_N == 90320
    seen = set(zip(((off + np.uint64(base)) % np.uint64(128)).tolist(), ln.tolist()))
    assert all((r, k) in seen for r in range(128) for k in range(705))
    for k in mc.SHA_LONG_LENGTHS:
        assert all((r, k) in seen for r in mc.SHA_LONG_RESIDUES)
    # in offset order no message begins before its predecessor ends, and the last ends inside the blob
    o, k = off.astype(np.int64), ln.astype(np.int64)
    assert (np.diff(o) >= 0).all() and (o[1:] >= o[:-1] + k[:-1]).all()
    assert (o[1:] - (o[:-1] + k[:-1]) < 128).all()  # the lowest free position with its residue
    assert o[-1] + k[-1] == len(blob) <= mc.sha_sweep_max_bytes()
    # both sides of the bucket clamp, and a lane count that fills no wave, block or bitmap word
    raw = (ln.astype(np.int64) + 8) // 64 + 1
    assert mc.sha_blocks(ln).max() == 1023 and {1023, 1024, 1025, 3126} <= set(raw.tolist())
    # gaps are random too: a byte read from outside a message changes its digest
    assert len(np.unique(blob[:4096])) > 200


def test_sha_sweep_reaches_every_ring_state():
    """The coverage in k_sha256_ring's own terms (sha256_kernels.hip): D0 the
    message's first dword in its line, sh its byte shift, block blk's window
    at ring position (D0 + 16 blk) & 63, the tail's at nfull, rem tail bytes."""
    _, off, ln = mc.sha_sweep(0)
    dense = slice(0, 128 * 705)
    r, k = (off[dense] % np.uint64(128)).astype(np.int64), ln[dense].astype(np.int64)
    d0, sh, nfull, rem = r >> 2, r & 3, k >> 6, k & 63
    tail_pos = (d0 + 16 * nfull) & 63
    # every tail window position x byte shift x tail length, position 63 (the window's 17th dword is the mirror's
    # last) included
    assert len(set(zip(tail_pos.tolist(), sh.tolist(), rem.tolist()))) == 64 * 4 * 64
    # full blocks 0..10: each at the 32 window positions of its phase x 4 shifts, together at all 64 positions
    full = set()
    for blk in range(11):
        has = nfull > blk
        here = set(zip(((d0[has] + 16 * blk) & 63).tolist(), sh[has].tolist()))
        assert len(here) == 32 * 4
        full |= here
    assert len(full) == 64 * 4
    # messages whose last byte is the last byte of a line, after every number of lines 1..6, and ones that end one
    # byte before and after it; the start-up cases: no line, one line, two lines, and a refill in the first block
    end = r + k
    for lines in range(1, 7):
        for e in (128 * lines - 1, 128 * lines, 128 * lines + 1):
            assert (end[k > 0] == e).any()
    nlines = (r + k + 127) >> 7
    assert {0, 1, 2, 3, 6} <= set(nlines.tolist()) and ((nlines == 0) & (k == 0) & (r == 0)).any()
    assert ((nlines == 1) & (k == 0)).any() and ((nlines == 1) & (nfull == 1)).any()


@pytest.mark.parametrize("kind", mc.KINDS)
def test_bound_messages_reach_the_encoder_bound(pb, kind):
    msgs, sorts = mc.gojson_bound_cases(kind)
    assert len(msgs) == 257 and {sorts.count(s) for s in ("bound", "minimal", "plain")} <= {85, 86}
    seen_lengths = set()
    for msg, sort in zip(msgs, sorts):
        pre = mc.encode(kind, msg)
        assert host_length(pb, kind, msg) == len(pre) <= slot_bound(kind, msg)
        if sort != "bound":
            continue
        fields = mc.string_fields(kind, msg)
        seen_lengths.update(len(s) for s in fields)
        six = 6 * sum(len(s) for s in fields)
        if kind == "preprepare":
            if msg[3] is not None:
                assert len(pre) == 188 + six == slot_bound(kind, msg) - 1
        else:
            assert len(pre) == mc.BOUND_BASE[kind] + six == slot_bound(kind, msg)
    assert seen_lengths == set(mc.BOUND_LENGTHS)
    if kind == "preprepare":
        nil = sum(m[3] is None for m in msgs)
        assert 40 <= nil <= 60 and any(m[3] is None and s == "bound" for m, s in zip(msgs, sorts))


@pytest.mark.parametrize("how", mc.LAYOUTS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_relayout_keeps_every_string(kind, how):
    from simple_pbft_amd.pbftv import PrePrepareColumns, ReplyColumns, RequestColumns, VoteColumns
    cls = {"request": RequestColumns, "vote": VoteColumns, "reply": ReplyColumns, "preprepare": PrePrepareColumns}
    n = 1100
    cols = cls[kind](mc.layout_batch(kind, n))
    out = mc.relayout(cols, how)
    names = mc.string_columns(cols)
    assert len(names) == {"request": 2, "vote": 2, "reply": 3, "preprepare": 3}[kind]
    assert out.args() != cols.args()
    for name in names:
        want = mc.column_strings(getattr(cols, name))
        blob, off, ln = getattr(out, name)
        assert mc.column_strings((blob, off, ln)) == want and len(want) == n
        assert blob.dtype == np.uint8 and off.dtype == np.uint64 and ln.dtype == np.uint32
        o, k = off.astype(np.int64), ln.astype(np.int64)
        live = k > 0
        assert (o[live] + k[live] <= len(blob)).all()
        assert (~live).sum() >= n // 7  # every seventh string of a column is empty
        if how == "reversed":
            assert o[live][-1] == 0 and (np.diff(o[live]) < 0).all()
        elif how == "interned":
            assert len(set(o[live].tolist())) == len(set(s for s in want if s))
            if name in ("digest", "node", "cid"):
                assert len(set(o[live].tolist())) <= 6  # offsets repeat (a pre-prepare's digest: 3 + 3 values)
        elif how == "gapped":
            assert o[live].min() >= 1000 and o[live][512:].min() > o[live][:512].max()
            assert (np.diff(o[live]) > k[live][:-1]).all()
        else:
            e = o[~live]
            assert (e[1::2] == len(blob)).all() and (e[0::2] < len(blob)).all() and (e[0::2] > 0).all()


def test_utf8_edges_encode_alike(pb):
    cols = mc.utf8_edge_strings()
    assert len(cols) == len(mc.UTF8_PREFIXES) == 9
    for col, (p, c) in zip(cols, mc.UTF8_PREFIXES):
        assert col[-1] == p  # the last string of the blob
        for q, d in mc.UTF8_PREFIXES:
            i = col.index(b"ab" + q)
            assert col[i + 1] == d + b"cd" and col[i + 2] == q and col[i + 3] == d
            # together the two strings are one valid sequence; apart, every byte of the prefix is U+FFFD
            assert gojson.string(q + d).count(b"\\ufffd") == 0
            assert gojson.string(q) == b'"' + b"\\ufffd" * len(q) + b'"'
            assert gojson.string(b"ab" + q) == b'"ab' + b"\\ufffd" * len(q) + b'"'
        for s in mc.UTF8_EXACT:
            assert s in col
        for kind in mc.KINDS:
            for msg in mc.utf8_messages(kind, col):
                assert host_encode(pb, kind, msg) == mc.encode(kind, msg)
    assert gojson.string(b"\xe2\x80\xa8") == b'"\\u2028"' and gojson.string(b"\xe2\x80\xa9") == b'"\\u2029"'
    assert gojson.string(b"\xef\xbf\xbd") == b'"\xef\xbf\xbd"'


def test_long_string_cases_shape(pb):
    cases = mc.long_string_cases()
    for kind in mc.KINDS:
        msgs = cases[kind]
        assert 64 < len(msgs) <= 80
        longest = sorted(max(len(s) for s in mc.string_fields(kind, m) or [b""]) for m in msgs)
        assert set(mc.LONG_LENGTHS) <= set(longest) and longest[0] < 24
    zero = [m for m in cases["request"] if m[2] == bytes(65536)]
    assert len(zero) == 1 and len(mc.encode("request", zero[0])) > 393000
    # the host encoder agrees on the long fields (one per kind is enough here: the GPU tests take them all)
    for kind in mc.KINDS:
        m = max(cases[kind], key=lambda m: len(mc.encode(kind, m)))
        assert host_encode(pb, kind, m) == mc.encode(kind, m)


def test_verify_msg_edges_shape(oracle_lib):
    import hashlib
    right = lambda j: hashlib.sha256(b"%d" % j).hexdigest().encode()  # noqa: E731
    rows = mc.verify_msg_edges(right)
    k = len(rows)
    idx = [r[5] for r in rows]
    assert {0, k - 1, k, 0xFFFFFFFF} <= set(idx) and all(i == j for j, i in enumerate(idx) if i < k)
    assert {len(r[4]) for r in rows} >= {0, 63, 64, 65}
    assert {r[1] for r in rows} >= {-1, mc.I64_MIN, mc.I64_MAX} and {r[3] for r in rows} == {mc.I64_MIN, -1, 0, 5,
                                                                                           mc.I64_MAX}
    for ch in b"/:`g":
        assert any(ch in r[4] for r in rows)
    bits = [oracle_lib.oracle_verify_msg(sv, last, bytes.fromhex(right(j).decode()), view, seq, d, len(d)) == 1
            for j, (sv, last, view, seq, d, _) in enumerate(rows)]
    assert bits[0] and bits[k - 1] and all(bits[j] for j in range(k) if idx[j] >= k)
    assert 20 < sum(bits) < k - 100  # both outcomes, neither rare
