"""pbftv_seal_votes / _replies / _preprepares on the GPU: every byte of the
blob, every offset, length, digest and ok bit against oracle/gojson.py's
*_signed forms around tests/rfc6979_model.py's signatures (tests/seal_cases.py);
the offsets scan at its block and chunk seams and, alone in a probe, at its
64-bit carries; unsigned rows, the capacity protocol, the argument checks, the
round trip through the flushes, two logical devices and the string columns'
freedoms."""
from __future__ import annotations

import base64
import ctypes
import glob
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import msgpath_cases as mc
import rfc6979_model as model
import seal_cases as cases
import sign_cases as sc
from conftest import ROOT
from simple_pbft_amd import DerColumn, Verifier
from simple_pbft_amd.pbftv import (PBFTV_EINVAL, PBFTV_ENOSIGNKEYS, PBFTV_ENOSPACE, PBFTV_OK, SIG_DER, SIG_RS,
                                   PbftvError, ReplyColumns, Sealed, VoteColumns)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257]
T, B = 256, 256  # wire.h kScanBlock, kScanChunk (checked against the probe below)
BIG = 0xFFFFFFFF
POISON = 0xA5
FMT = {"rs": SIG_RS, "der": SIG_DER}


@pytest.fixture(scope="module")
def ver():
    """seal_cases' five signing keys and, as verify keys, their public halves"""
    ds = sc.keypool(cases.NKEYS)
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).all()
        assert v.register_keys(sc.pubkeys(ds)).all()
        yield v


def req_sig_column(rsigs):
    """(blob, off, len, nil) of a pre-prepare batch's client signatures"""
    blob, off, ln = Verifier.pack([s or b"" for s in rsigs])
    return blob, off, ln, np.array([s is None for s in rsigs], np.uint8)


def raw_seal(v, kind, cols, rcol, kidx, fmt, cap, slack=64, digests=True, okbits=True):
    """The C call with every output poisoned first.  Returns (rc, blob buffer of
    cap + slack bytes, off, len, total, digests, raw bitmap bytes)."""
    n = cols.n
    kidx = np.ascontiguousarray(kidx, np.uint32)
    blob = np.full(cap + slack, POISON, np.uint8)
    off = np.full(n + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)
    ln = np.full(n + 1, 0xEEEEEEEE, np.uint32)
    dg = np.full((n + 1, 32), POISON, np.uint8)
    bm = np.full((n + 7) // 8 + 8, 0xFF, np.uint8)
    total = ctypes.c_uint64(0xEEEE)
    args = list(cols.args())
    if kind == "preprepare":
        args += [None] * 4 if rcol is None else [a.ctypes.data for a in rcol]
    fn = getattr(v._L, {"vote": "pbftv_seal_votes", "reply": "pbftv_seal_replies",
                        "preprepare": "pbftv_seal_preprepares"}[kind])
    rc = fn(v._h, n, *args, kidx.ctypes.data, fmt, blob.ctypes.data, cap, off.ctypes.data, ln.ctypes.data,
            ctypes.byref(total), dg.ctypes.data if digests else None, bm.ctypes.data if okbits else None)
    return rc, blob, off, ln, total.value, dg, bm


def check_raw(res, wires, want_digests, cap):
    """A successful raw call against the expected wire forms (b"": unsigned):
    nothing past the total, the arrays' ends or the bitmap's bytes is written."""
    rc, blob, off, ln, total, dg, bm = res
    n = len(wires)
    assert rc == PBFTV_OK
    assert total == sum(map(len, wires)) <= cap
    assert (off[n:] == 0xEEEEEEEEEEEEEEEE).all() and (ln[n:] == 0xEEEEEEEE).all() and (dg[n:] == POISON).all()
    assert (blob[total:] == POISON).all()
    nb = (n + 7) // 8
    bits = np.unpackbits(bm[:nb], bitorder="little")
    assert not bits[n:].any() and (bm[nb:] == 0xFF).all()
    cases.check_layout(Sealed(blob[:total], off[:n], ln[:n], dg[:n], bits[:n].astype(bool)), wires)
    if want_digests is not None:
        assert (dg[:n] == want_digests).all()


# ---------------------------------------------------------------- byte-exact, small
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", ["rs", "der"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_sealed_bytes_match_the_oracle(ver, kind, fmt, n):
    msgs, rsigs, kidx = cases.batch(kind, n)
    wires, digests = cases.expected(kind, n, fmt == "der")
    cols = cases.columns(kind, msgs)
    rcol = req_sig_column(rsigs) if kind == "preprepare" else None
    cap = sum(map(len, wires))
    check_raw(raw_seal(ver, kind, cols, rcol, kidx, FMT[fmt], cap), wires, digests, cap)


def test_binding_and_optional_outputs(ver):
    n = 65
    msgs, rsigs, kidx = cases.batch("preprepare", n)
    wires, digests = cases.expected("preprepare", n, True)
    cols = cases.columns("preprepare", msgs)
    s = ver.seal_preprepares(cols, rsigs, kidx, SIG_DER)
    cases.check_layout(s, wires)
    assert (s.digests == digests).all() and s.messages() == wires and len(s) == n
    assert ver.seal_preprepares(cols, rsigs, kidx, SIG_DER, digests=False).digests is None
    # no digests, no bitmap: the same bytes
    rc, blob, off, ln, total, dg, bm = raw_seal(ver, "preprepare", cols, req_sig_column(rsigs), kidx, SIG_DER,
                                                len(s.blob), digests=False, okbits=False)
    assert rc == PBFTV_OK and blob[:total].tobytes() == b"".join(wires) and (dg == POISON).all() and (bm == 0xFF).all()
    # a NULL client-signature column: every embedded request's signature is null
    nil = ver.seal_preprepares(cols, None, kidx, SIG_RS)
    want, _ = cases.expected("preprepare", n, False)
    for i in range(n):
        sig = cases.signed("preprepare")[i % cases.DISTINCT][1]
        assert nil[i] == cases.wire("preprepare", msgs[i], None, sig), i
    assert any(a != b for a, b in zip(nil.messages(), want))


# ---------------------------------------------------------------- scan seams
SEAM_SIZES = [T - 1, T, T + 1, T * B - 1, T * B, T * B + 1, 2 * T * B + T + 3]


def _plain_vote(i: int):
    return (i % 13, i, b"%0*x" % (1 + i % 64, i * 2654435761 % (1 << 4 * (1 + i % 64))), b"n" * (i % 5) + b"%d" % i,
            i % 3)


@pytest.fixture(scope="module")
def seam_votes(ver):
    """The largest seam batch once: plain-ASCII votes of varying length (every
    shorter batch is a prefix), their digests from hashlib, their signatures
    from the library's own sign_batch -- 64 sampled rows against the model."""
    n = max(SEAM_SIZES)
    votes = [_plain_vote(i) for i in range(n)]
    pre = [b'{"viewID":%d,"sequenceID":%d,"digest":"%s","nodeID":"%s","msgType":%d' % v for v in votes]
    digests = np.frombuffer(b"".join(hashlib.sha256(p + b"}").digest() for p in pre), np.uint8).reshape(n, 32)
    kidx = (np.arange(n) * 7 % cases.NKEYS).astype(np.uint32)
    sigs, ok = ver.sign_batch(digests, kidx)
    assert ok.all()
    ds = sc.keypool(cases.NKEYS)
    for i in np.random.default_rng(64).choice(n, 64, replace=False).tolist() + [0, n - 1]:
        assert sigs[i].tobytes() == model.sign_bytes(digests[i].tobytes(), ds[kidx[i]]), i
    wires = [p + b',"signature":"' + base64.b64encode(sigs[i].tobytes()) + b'"}' for i, p in enumerate(pre)]
    return votes, kidx, wires, digests


@pytest.mark.parametrize("n", SEAM_SIZES)
def test_offsets_at_the_scan_seams(ver, seam_votes, n):
    votes, kidx, wires, digests = seam_votes
    s = ver.seal_votes(VoteColumns(votes[:n]), kidx[:n])
    lens = np.array([len(w) for w in wires[:n]], np.uint64)
    assert s.len.tolist() == lens.tolist() and len(set(lens.tolist())) > 40
    cs = np.cumsum(lens, dtype=np.uint64)
    assert s.off[0] == 0 and (s.off[1:] == cs[:-1]).all() and len(s.blob) == int(cs[-1])
    assert s.ok.all() and (s.digests == digests[:n]).all()
    assert s.blob.tobytes() == b"".join(wires[:n])


@pytest.fixture(scope="module")
def probe():
    d = os.path.join(ROOT, "tests", "cpp")
    so, src = os.path.join(d, "libseal_probe.so"), os.path.join(d, "seal_probe.hip")
    deps = [src] + glob.glob(os.path.join(ROOT, "simple_pbft_amd", "csrc", "*.h")) + \
        [os.path.join(ROOT, "simple_pbft_amd", "csrc", "seal_kernels.hip")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as __graft_entry__.build() and the Makefile
        if not shutil.which(hipcc):
            pytest.fail("tests/cpp/libseal_probe.so is missing or older than its sources and there is no hipcc "
                        "to build it: run __graft_entry__.build()")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                        "-shared", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.sealp_offsets.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.sealp_scan_block.restype = lib.sealp_scan_chunk.restype = ctypes.c_uint32
    assert (lib.sealp_scan_block(), lib.sealp_scan_chunk()) == (T, B)
    return lib


def _carry_lengths():
    big = [2 ** 31 + 1000, 2 ** 32 - 1, 2 ** 31 + 12345]  # (the second list takes up to T off each: still >= 2^31)
    out = {"three": [0, big[0], 0, 0, big[1], 7, big[2], 0]}
    row = []
    for i in range(T + 1):  # T + 1 large lengths, zeros and small ones between them: more than one block of each
        row += [big[i % 3] - i, 0] + ([3] if i % 4 == 0 else [])
    out["block+1"] = row
    out["chunks"] = [(big[i % 3] if i % T == T - 1 else i % 2) for i in range(T * B + T + 5)]  # carry across the chunk
    return out


@pytest.mark.parametrize("which", ["three", "block+1", "chunks"])
def test_offsets_carry_past_32_bits(probe, which):
    lens = _carry_lengths()[which]
    n = len(lens)
    ln = np.array(lens, np.uint32)
    off = np.full(n + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)
    total = np.zeros(1, np.uint64)
    assert probe.sealp_offsets(ln.ctypes.data, n, off.ctypes.data, total.ctypes.data) == 0
    want, t = [], 0
    for x in lens:  # Python integers
        want.append(t)
        t += x
    assert t > 2 ** 33 and int(total[0]) == t
    assert off[:n].tolist() == want and off[n] == 0xEEEEEEEEEEEEEEEE


# ---------------------------------------------------------------- unsigned rows
def test_unsigned_rows_write_nothing_and_leave_their_neighbours_alone():
    """An index past the key set and a key d = 0 among valid rows, at the first
    and last positions and on both sides of the 256-lane block seams."""
    ds = list(sc.keypool(cases.NKEYS)) + [0]
    n = 600
    bad = {0: cases.NKEYS, 1: BIG, 255: cases.NKEYS + 1, 256: cases.NKEYS, 257: 1 << 31, 511: BIG, 512: cases.NKEYS,
           n - 1: cases.NKEYS}
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).tolist() == [True] * cases.NKEYS + [False]
        for kind, fmt in (("vote", "rs"), ("reply", "der"), ("preprepare", "der")):
            msgs, rsigs, kidx = cases.batch(kind, n)
            wires, digests = cases.expected(kind, n, fmt == "der")
            kidx = kidx.copy()
            for i, j in bad.items():
                kidx[i] = j
                wires[i] = b""
            rcol = req_sig_column(rsigs) if kind == "preprepare" else None
            cap = sum(map(len, wires))
            res = raw_seal(v, kind, cases.columns(kind, msgs), rcol, kidx, FMT[fmt], cap)
            check_raw(res, wires, digests, cap)  # (the digests are those of every row, signed or not)
            assert [int(x) == 0 for x in res[3][:n]] == [i in bad for i in range(n)]
        # every row unsigned: a total of 0, nothing written
        msgs, _, kidx = cases.batch("vote", 70)
        res = raw_seal(v, "vote", cases.columns("vote", msgs), None, np.full(70, BIG, np.uint32), SIG_RS, 0)
        check_raw(res, [b""] * 70, None, 0)


# ---------------------------------------------------------------- capacity and arguments
@pytest.mark.parametrize("kind", cases.KINDS)
def test_capacity_protocol(ver, kind):
    n = 257
    msgs, rsigs, kidx = cases.batch(kind, n)
    wires, digests = cases.expected(kind, n, True)
    cols = cases.columns(kind, msgs)
    rcol = req_sig_column(rsigs) if kind == "preprepare" else None
    total = sum(map(len, wires))
    for cap in (total - 1, 0):
        rc, blob, off, ln, got_total, dg, bm = raw_seal(ver, kind, cols, rcol, kidx, SIG_DER, cap)
        assert rc == PBFTV_ENOSPACE and got_total == total
        assert (blob == POISON).all()  # nothing written to out_wire
        lens = [len(w) for w in wires]
        assert ln[:n].tolist() == lens and off[:n].tolist() == [sum(lens[:i]) for i in range(n)]
        assert (dg[:n] == digests).all()
        assert np.unpackbits(bm[:(n + 7) // 8], bitorder="little")[:n].all()
    check_raw(raw_seal(ver, kind, cols, rcol, kidx, SIG_DER, total), wires, digests, total)
    assert b"too small" in ver._L.pbftv_strerror(PBFTV_ENOSPACE)
    with pytest.raises(PbftvError) as ei:
        ver._seal(getattr(ver._L, "pbftv_seal_votes"), 3, VoteColumns(cases.batch("vote", 3)[0]).args(),
                  np.zeros(3, np.uint32), SIG_RS, True, 10)
    assert ei.value.code == PBFTV_ENOSPACE


def test_argument_checks(ver):
    L, c = ver._L, ver._h
    n = 4
    msgs, _, kidx = cases.batch("vote", n)
    cols = VoteColumns(msgs)
    blob, off, ln = np.full(4096, POISON, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    total = ctypes.c_uint64(77)
    tp = ctypes.byref(total)
    bp, op, lp, kp = blob.ctypes.data, off.ctypes.data, ln.ctypes.data, kidx.ctypes.data
    a = cols.args()

    def votes(ctx=c, n=n, a=a, kp=kp, fmt=SIG_RS, bp=bp, cap=4096, op=op, lp=lp, tp=tp):
        return L.pbftv_seal_votes(ctx, n, *a, kp, fmt, bp, cap, op, lp, tp, None, None)

    assert votes() == PBFTV_OK and total.value == int(ln.sum()) > 0
    total.value = 77
    assert votes(n=0) == PBFTV_OK and total.value == 0  # n = 0 writes only the total
    assert votes(n=0, a=[None] * 9, kp=None, bp=None, cap=0, op=None, lp=None) == PBFTV_OK
    assert votes(n=1 << 32) == PBFTV_EINVAL
    for fmt in (-1, 2, 7):
        assert votes(fmt=fmt) == PBFTV_EINVAL
    assert votes(ctx=None) == PBFTV_EINVAL
    assert votes(kp=None) == PBFTV_EINVAL
    assert votes(op=None) == PBFTV_EINVAL
    assert votes(lp=None) == PBFTV_EINVAL
    assert votes(tp=None) == PBFTV_EINVAL
    assert votes(bp=None) == PBFTV_EINVAL
    for k in (0, 1, 3, 4, 6, 7, 8):  # every column pointer but the two string blobs
        assert votes(a=a[:k] + [None] + a[k + 1:]) == PBFTV_EINVAL, k
    # replies and pre-prepares: a missing column, and a client-signature column without its offsets
    rmsgs, _, _ = cases.batch("reply", n)
    ra = ReplyColumns(rmsgs).args()
    assert L.pbftv_seal_replies(c, n, *ra, kp, SIG_RS, bp, 4096, op, lp, tp, None, None) == PBFTV_OK
    assert L.pbftv_seal_replies(c, n, *([None] + ra[1:]), kp, SIG_RS, bp, 4096, op, lp, tp, None, None) == PBFTV_EINVAL
    pmsgs, prs, _ = cases.batch("preprepare", n)
    pa = cases.columns("preprepare", pmsgs).args()
    rb, ro, rl, rn = (x.ctypes.data for x in req_sig_column(prs))
    pp = L.pbftv_seal_preprepares
    assert pp(c, n, *pa, rb, ro, rl, rn, kp, SIG_DER, bp, 4096, op, lp, tp, None, None) == PBFTV_OK
    assert pp(c, n, *pa, rb, None, rl, rn, kp, SIG_DER, bp, 4096, op, lp, tp, None, None) == PBFTV_EINVAL
    assert pp(c, n, *pa, rb, ro, None, rn, kp, SIG_DER, bp, 4096, op, lp, tp, None, None) == PBFTV_EINVAL
    assert pp(c, n, *pa, None, None, None, None, kp, SIG_DER, bp, 4096, op, lp, tp, None, None) == PBFTV_OK
    assert pp(c, n, *(pa[:5] + [None] + pa[6:]), rb, ro, rl, rn, kp, SIG_DER, bp, 4096, op, lp, tp, None,
              None) == PBFTV_EINVAL  # has_request
    with Verifier(device_mask=1) as fresh:
        f = fresh._h
        assert votes(ctx=f) == PBFTV_ENOSIGNKEYS
        assert L.pbftv_seal_replies(f, n, *ra, kp, SIG_RS, bp, 4096, op, lp, tp, None, None) == PBFTV_ENOSIGNKEYS
        assert pp(f, n, *pa, rb, ro, rl, rn, kp, SIG_DER, bp, 4096, op, lp, tp, None, None) == PBFTV_ENOSIGNKEYS
        assert votes(ctx=f, n=0) == PBFTV_OK


# ---------------------------------------------------------------- round trip through the receive side
def _parse(kind, wire_bytes):
    m = json.loads(wire_bytes)
    sig = base64.b64decode(m["signature"])
    if kind == "vote":
        return (m["viewID"], m["sequenceID"], m["digest"].encode(), m["nodeID"].encode(), m["msgType"]), sig
    return (m["viewID"], m["timestamp"], m["clientID"].encode(), m["nodeID"].encode(), m["result"].encode()), sig


@pytest.mark.parametrize("fmt", ["rs", "der"])
@pytest.mark.parametrize("kind", ["vote", "reply"])
def test_sealed_messages_pass_the_flushes(ver, kind, fmt):
    n = 300
    if kind == "vote":
        msgs = [(i % 5, i, hashlib.sha256(b"r%d" % (i % 9)).hexdigest().encode(), b"node%d" % (i % 4), 1 + i % 2)
                for i in range(n)]
    else:
        msgs = [(i % 5, 10 ** 15 + i, b"client%d" % (i % 7), b"node%d" % (i % 4), b"Executed %d" % i)
                for i in range(n)]
    kidx = (np.arange(n) * 3 % cases.NKEYS).astype(np.uint32)
    cols = cases.columns(kind, msgs)
    s = (ver.seal_votes if kind == "vote" else ver.seal_replies)(cols, kidx, FMT[fmt])
    assert s.ok.all()
    parsed = [_parse(kind, w) for w in s.messages()]
    assert [p[0] for p in parsed] == msgs
    sigs = [p[1] for p in parsed]
    flip = 137
    bad = bytearray(sigs[flip])
    bad[len(bad) - 5] ^= 0x04  # inside s: still a well-formed encoding
    sigs[flip] = bytes(bad)
    back = cases.columns(kind, [p[0] for p in parsed])
    if fmt == "rs":
        S = np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64)
        got = (ver.flush_votes(back, S, kidx) if kind == "vote" else ver.flush_replies(back, S, kidx))[:2]
    else:
        col = DerColumn(ders=sigs)
        got = (ver.flush_votes_der(back, col, kidx) if kind == "vote" else ver.flush_replies_der(back, col, kidx))[:2]
    dg, ok = got
    assert (dg == s.digests).all()
    assert ok.tolist() == [i != flip for i in range(n)]


# ---------------------------------------------------------------- two logical devices
@pytest.fixture
def two_devices(monkeypatch):
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    v = Verifier()
    assert v.device_count() == 2 and v.device_id(0) == v.device_id(1)
    assert v.register_signing_keys(sc.col(sc.keypool(cases.NKEYS))).all()
    yield v
    v.close()


@pytest.mark.parametrize("n", [513, 2049, 5000])
def test_two_devices_give_one_devices_bytes(ver, two_devices, n):
    for kind, fmt in (("vote", SIG_RS), ("preprepare", SIG_DER), ("reply", SIG_DER)):
        msgs, rsigs, kidx = cases.batch(kind, n)
        kidx = kidx.copy()
        kidx[[0, 511, 512, n - 1]] = BIG  # unsigned rows at the ends and on both sides of the shard seam
        cols = cases.columns(kind, msgs)
        rcol = req_sig_column(rsigs) if kind == "preprepare" else None
        one = raw_seal(ver, kind, cols, rcol, kidx, fmt, 1 << 22)
        two = raw_seal(two_devices, kind, cols, rcol, kidx, fmt, 1 << 22)
        assert one[0] == two[0] == PBFTV_OK and one[4] == two[4] > 0
        for a, b in zip(one[1:], two[1:]):
            assert np.array_equal(a, b)
        off, ln = two[2][:n], two[3][:n].astype(np.uint64)
        assert off[0] == 0 and (off[1:] == np.cumsum(ln)[:-1]).all()  # global offsets
        # ... and the capacity protocol across shards: the whole total, global offsets, an untouched blob
        short = raw_seal(two_devices, kind, cols, rcol, kidx, fmt, one[4] - 1)
        assert short[0] == PBFTV_ENOSPACE and short[4] == one[4] and (short[1] == POISON).all()
        assert np.array_equal(short[2], one[2]) and np.array_equal(short[3], one[3])
    # the first rows against the oracle, so that "equal" is not "equally wrong"
    wires, _ = cases.expected("reply", 64, True)
    assert [two[1][int(two[2][i]):int(two[2][i]) + int(two[3][i])].tobytes() for i in range(1, 64)] == wires[1:]


# ---------------------------------------------------------------- string-column conventions
@pytest.mark.parametrize("how", mc.LAYOUTS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_string_column_layouts_give_the_same_bytes(ver, kind, how):
    n = 257
    msgs = mc.layout_batch(kind, n)
    kidx = (np.arange(n) * 3 % cases.NKEYS).astype(np.uint32)
    packed = cases.columns(kind, msgs)
    rsigs = None
    if kind == "preprepare":
        rng = np.random.default_rng(0x1A7)
        rsigs = [None if i % 5 == 4 else (b"" if i % 5 == 3 else rng.bytes(cases.SIG_LENS[i % 11])) for i in range(n)]
        want = ver.seal_preprepares(packed, rsigs, kidx, SIG_DER)
    else:
        want = (ver.seal_votes if kind == "vote" else ver.seal_replies)(packed, kidx, SIG_DER)
    assert want.ok.all()
    # the packed result is the oracle's around the library's own DER signatures over hashlib's digests
    pre = [cases.preimage(kind, m) for m in msgs]
    dg = np.frombuffer(b"".join(hashlib.sha256(p).digest() for p in pre), np.uint8).reshape(n, 32)
    der, dl = ver.sign_der_batch(dg, kidx)
    for i in range(n):
        assert want[i] == cases.wire(kind, msgs[i], rsigs[i] if rsigs else None, der[i, :dl[i]].tobytes()), i
    cols = mc.relayout(packed, how)
    rcol = None
    if kind == "preprepare":
        rb, ro, rl = mc._layout([s or b"" for s in rsigs], how, np.random.default_rng(5))
        rn = np.array([s is None for s in rsigs], np.uint8)
        if how == "empties":  # the rows the call must not read hold wild offsets too: nil ones, those without a request
            ro = ro.copy()
            ro[[i for i in range(n) if rsigs[i] is None or msgs[i][3] is None or not rsigs[i]]] = BIG << 20
        rcol = (rb, ro, rl, rn)
    res = raw_seal(ver, kind, cols, rcol, kidx, SIG_DER, len(want.blob))
    check_raw(res, want.messages(), dg, len(want.blob))
