"""The device Go-JSON encoder (gojson_kernels.hip) and the column packing in
front of it (pbftv_api.cpp Packer::add_str) at their seams, with the inputs
of tests/msgpath_cases.py:

  * messages that fill their slot (request_bound, vote_bound, reply_bound) to
    the last byte, next to minimal and plain ones, across a 256-lane block:
    a bound one byte short would let a lane write its neighbour's first byte;
  * truncated UTF-8 at the end of a string whose successor in the blob begins
    with the completing bytes; strings of up to 70,001 bytes; one 393 KB preimage;
  * string columns laid out reversed, interned, gapped and with stray offsets
    for empty strings, on one device and on two logical devices (shards of
    1024 + 76 messages);
  * State.verifyMsg at the int64 extremes, with digests of length 0 / 63 / 64 /
    65, upper case, one digit wrong, characters next to the hex ranges, and
    state indices 0, k - 1, k and 0xFFFFFFFF.

Expected digests are hashlib's SHA-256 of oracle/gojson.py's encoding;
message bits come from the oracle's verifyMsg, signature bits from the
oracle's ECDSA verify.  Bit-exact for every digest and every bit."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import msgpath_cases as mc
from oracle import gojson
from test_gpu_messages import _keys, _oracle_bits, _signed, hexes, sha

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    from simple_pbft_amd import Verifier
    v = Verifier()
    yield v
    v.close()


def columns(kind, msgs):
    from simple_pbft_amd.pbftv import PrePrepareColumns, ReplyColumns, RequestColumns, VoteColumns
    return {"request": RequestColumns, "vote": VoteColumns, "reply": ReplyColumns,
            "preprepare": PrePrepareColumns}[kind](msgs)


def digest_call(ver, kind, msgs):
    return hexes(getattr(ver, f"digest_{kind}_batch")(msgs))


def want_digests(kind, msgs):
    return [sha(mc.encode(kind, m)) for m in msgs]


def assert_digests(got, want, what):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, f"{what}: messages {bad[:12]} of {len(want)} differ"


# ------------------------------------------------------------------ slot bounds
@pytest.mark.parametrize("kind", mc.KINDS)
def test_bound_cases_digest_calls(ver, kind):
    msgs, _ = mc.gojson_bound_cases(kind)
    assert_digests(digest_call(ver, kind, msgs), want_digests(kind, msgs), kind)


def test_bound_cases_flush_requests_both_slot_sets(ver):
    """assigned_seqs alternate between -2^63 and 0: the consensus preimages
    (slots [n, 2n)) of the at-bound requests are at their bound too."""
    msgs, sorts = mc.gojson_bound_cases("request")
    n = len(msgs)
    assigned = np.where(np.arange(n) % 2 == 0, mc.I64_MIN, 0).astype(np.int64)
    assert any(s == "bound" and a == mc.I64_MIN for s, a in zip(sorts, assigned))
    dg, ok, cons = ver.flush_requests(columns("request", msgs), assigned_seqs=assigned)
    assert ok is None
    assert_digests(hexes(dg), want_digests("request", msgs), "as sent")
    assert_digests(hexes(cons), [sha(gojson.request(m[0], m[1], m[2], int(a))) for m, a in zip(msgs, assigned)],
                   "consensus")


def test_bound_cases_flush_preprepares_pair(ver):
    """The pair kernel: pre-prepare preimages in slots [0, n), their requests' in [n, 2n)."""
    msgs, _ = mc.gojson_bound_cases("preprepare")
    dg, rdg, ok, mok = ver.flush_preprepares(columns("preprepare", msgs), req_digests=True)
    assert ok is None and mok is None
    assert_digests(hexes(dg), want_digests("preprepare", msgs), "pre-prepare")
    assert_digests(hexes(rdg), [sha(gojson.request_or_null(m[3])) for m in msgs], "request")


# ------------------------------------------------------------------ UTF-8 edges, long strings
@pytest.mark.parametrize("kind", mc.KINDS)
def test_utf8_edges(ver, kind):
    for col in mc.utf8_edge_strings():
        msgs = mc.utf8_messages(kind, col)
        assert_digests(digest_call(ver, kind, msgs), want_digests(kind, msgs), f"{kind}, last string {col[-1]!r}")


@pytest.fixture(scope="module")
def long_cases():
    cases = mc.long_string_cases()
    return {kind: (msgs, [mc.encode(kind, m) for m in msgs]) for kind, msgs in cases.items()}


@pytest.mark.parametrize("kind", mc.KINDS)
def test_long_strings_digest_calls(ver, long_cases, kind):
    msgs, pre = long_cases[kind]
    assert max(map(len, pre)) > (390000 if kind in ("request", "preprepare") else 70000)
    assert_digests(digest_call(ver, kind, msgs), [sha(p) for p in pre], kind)


def test_long_strings_flush_replies(ver, oracle_lib, long_cases):
    rng = np.random.default_rng(0x10F1)
    privs, keys = _keys(oracle_lib, rng, 3)
    assert ver.register_keys(keys).all()
    msgs, pre = long_cases["reply"]
    S, K, H = _signed(oracle_lib, rng, pre, privs)
    dg, ok = ver.flush_replies(columns("reply", msgs), S, K)
    assert_digests(hexes(dg), [sha(p) for p in pre], "reply")
    assert ok.tolist() == _oracle_bits(oracle_lib, H, S, K, keys) and ok.any() and not ok.all()


def test_long_strings_flush_requests(ver, oracle_lib, long_cases):
    rng = np.random.default_rng(0x10F2)
    privs, keys = _keys(oracle_lib, rng, 3)
    assert ver.register_keys(keys).all()
    msgs, pre = long_cases["request"]
    S, K, H = _signed(oracle_lib, rng, pre, privs)
    assigned = np.arange(len(msgs), dtype=np.int64) * 1000003 - 5
    dg, ok, cons = ver.flush_requests(columns("request", msgs), S, K, assigned)
    assert_digests(hexes(dg), [sha(p) for p in pre], "as sent")
    assert ok.tolist() == _oracle_bits(oracle_lib, H, S, K, keys) and ok.any() and not ok.all()
    assert_digests(hexes(cons), [sha(gojson.request(m[0], m[1], m[2], int(a))) for m, a in zip(msgs, assigned)],
                   "consensus")


# ------------------------------------------------------------------ column layouts
N_LAYOUT = 1100  # two logical devices: shards of 1024 + 76, above the 512 shard alignment


@pytest.fixture(scope="module")
def layout_cases(oracle_lib):
    return build_layout_cases(oracle_lib)


def build_layout_cases(oracle_lib):
    """kind -> its messages and the expected outputs of its flush, computed once."""
    n = N_LAYOUT
    out = {}
    for kind in mc.KINDS:
        msgs = mc.layout_batch(kind, n)
        out[kind] = {"msgs": msgs, "digests": want_digests(kind, msgs)}
    # votes: 11 states (view = index), state index 11 out of range
    k = 11
    s_view = np.arange(k, dtype=np.int64)
    s_last = np.array([-1, 500, -1, 2000, 7, -1, 0, 1099, -1, 300, 900], np.int64)
    digs = sorted({m[2] for m in out["vote"]["msgs"] if m[2]})
    s_dig = np.frombuffer(b"".join(bytes.fromhex(digs[j % 3].decode()) for j in range(k)), np.uint8).reshape(k, 32)
    sidx = np.array([(i * 7) % (k + 1) if i % 3 else i % 11 for i in range(n)], np.uint32)
    want = []
    for (view, seq, d, _, _), st in zip(out["vote"]["msgs"], sidx.tolist()):
        want.append(st < k and oracle_lib.oracle_verify_msg(int(s_view[st]), int(s_last[st]), s_dig[st].tobytes(),
                                                            view, seq, d, len(d)) == 1)
    assert 50 < sum(want) < n - 50
    out["vote"].update(states=(s_view, s_last, s_dig.copy()), sidx=sidx, msg_ok=want)
    want = []
    for (view, seq, d, req), st in zip(out["preprepare"]["msgs"], sidx.tolist()):
        qd = hashlib.sha256(gojson.request_or_null(req)).digest()
        want.append(st < k and oracle_lib.oracle_verify_msg(int(s_view[st]), int(s_last[st]), qd, view, seq, d,
                                                            len(d)) == 1)
    assert 50 < sum(want) < n - 50
    out["preprepare"].update(states=(s_view, s_last), sidx=sidx, msg_ok=want,
                             req_digests=[sha(gojson.request_or_null(m[3])) for m in out["preprepare"]["msgs"]])
    assigned = np.arange(n, dtype=np.int64) * 3 - 1000
    out["request"].update(assigned=assigned, consensus=[sha(gojson.request(m[0], m[1], m[2], int(a)))
                                                        for m, a in zip(out["request"]["msgs"], assigned)])
    return out


def check_layouts(v, cases):
    for kind in mc.KINDS:
        c = cases[kind]
        packed = columns(kind, c["msgs"])
        for how in ("packed",) + mc.LAYOUTS:
            cols = packed if how == "packed" else mc.relayout(packed, how)
            what = f"{kind}, {how}"
            if kind == "request":
                dg, _, cons = v.flush_requests(cols, assigned_seqs=c["assigned"])
                assert_digests(hexes(cons), c["consensus"], what + ", consensus")
            elif kind == "vote":
                dg, _, mok = v.flush_votes(cols, states=c["states"], state_idx=c["sidx"])
                assert mok.tolist() == c["msg_ok"], what
            elif kind == "reply":
                dg, _ = v.flush_replies(cols)
            else:
                dg, rdg, _, mok = v.flush_preprepares(cols, states=c["states"], state_idx=c["sidx"], req_digests=True)
                assert_digests(hexes(rdg), c["req_digests"], what + ", request")
                assert mok.tolist() == c["msg_ok"], what
            assert_digests(hexes(dg), c["digests"], what)


def test_layouts_one_device(ver, layout_cases):
    check_layouts(ver, layout_cases)


def test_layouts_two_logical_devices(layout_cases, monkeypatch):
    """PBFTV_ALIAS_DEVICES=2: add_str rebases each shard onto its own minimum
    offset (non-zero for the first shard of a reversed column, for the second
    of the others, for both of a gapped one)."""
    from simple_pbft_amd import Verifier
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    with Verifier(device_mask=1) as v:
        assert v.device_count() == 2
        check_layouts(v, layout_cases)


# ------------------------------------------------------------------ verifyMsg edges
def edge_states(rows):
    k = len(rows)
    assert {r[5] for r in rows} >= {0, k - 1, k, 0xFFFFFFFF}
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
            np.array([r[5] for r in rows], np.uint32))


def edge_bits(oracle_lib, rows, state_digest):
    k = len(rows)
    want = [idx < k and oracle_lib.oracle_verify_msg(sv, last, state_digest(j), view, seq, d, len(d)) == 1
            for j, (sv, last, view, seq, d, idx) in enumerate(rows)]
    assert want[0] and want[k - 1] and 20 < sum(want) < k - 100
    return want


def test_verify_msg_edges_votes(ver, oracle_lib):
    dig = lambda j: hashlib.sha256(b"state %d" % j).digest()  # noqa: E731
    rows = mc.verify_msg_edges(lambda j: dig(j).hex().encode())
    s_view, s_last, sidx = edge_states(rows)
    s_dig = np.frombuffer(b"".join(dig(j) for j in range(len(rows))), np.uint8).reshape(-1, 32)
    votes = [(view, seq, d, b"node%d" % (j % 4), j % 2) for j, (_, _, view, seq, d, _) in enumerate(rows)]
    dg, _, mok = ver.flush_votes(columns("vote", votes), states=(s_view, s_last, s_dig), state_idx=sidx)
    assert_digests(hexes(dg), want_digests("vote", votes), "vote")
    assert mok.tolist() == edge_bits(oracle_lib, rows, dig)


def test_verify_msg_edges_preprepares(ver, oracle_lib):
    req = lambda j: None if j % 5 == 2 else (j, b"c%d" % j, b"op", -j)  # noqa: E731
    dig = lambda j: hashlib.sha256(gojson.request_or_null(req(j))).digest()  # noqa: E731
    rows = mc.verify_msg_edges(lambda j: dig(j).hex().encode())
    s_view, s_last, sidx = edge_states(rows)
    pps = [(view, seq, d, req(j)) for j, (_, _, view, seq, d, _) in enumerate(rows)]
    dg, rdg, _, mok = ver.flush_preprepares(columns("preprepare", pps), states=(s_view, s_last), state_idx=sidx,
                                            req_digests=True)
    assert_digests(hexes(dg), want_digests("preprepare", pps), "pre-prepare")
    assert hexes(rdg) == [dig(j).hex() for j in range(len(rows))]
    assert mok.tolist() == edge_bits(oracle_lib, rows, dig)
