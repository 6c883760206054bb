"""pbftv_flush_requests_wirekey / pbftv_flush_replies_wirekey: client-signed
requests and replies with each message's key carried in the call (SEC1
compressed, or X||Y), one round trip -- digests against oracle/gojson.py +
hashlib, signature bits against the oracle under the key a Python big-integer
decode yields (tests/wirekey_cases.py).  Five client keys; about a third of the
messages are corrupted: a flipped r, another client's key, or a wrong-parity
prefix (which decodes to the negated key).  On a Verifier that never
registered keys, and across two logical devices."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import wirekey_cases as wc
from oracle import gojson
from simple_pbft_amd import KEY_SEC1_COMPRESSED, KEY_XY, Verifier
from simple_pbft_amd.pbftv import PBFTV_EINVAL, ReplyColumns, RequestColumns

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
ALPHABET = [b"x", b"Z", b"0", b"<", b">", b"&", b'"', b"\\", b"\t", b"\n", b"\x00", b"\x7f", b"\xe2\x80\xa8", b"\xff",
            b"\xc2\xa2", b"\xf0\x90\x80\x80", b"\xe2\x82", b"\xc0\x80", b"\xed\xa0\x80"]
INT_EDGES = [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 10 ** 18, 1668519247222762700]
FORMATS = [KEY_SEC1_COMPRESSED, KEY_XY]


@pytest.fixture(scope="module")
def ver():
    """pbftv_register_keys is never called on this context"""
    with Verifier(device_mask=1) as v:
        yield v


def rand_str(rng, maxlen=12):
    if rng.integers(0, 3) == 0:
        return rng.bytes(int(rng.integers(0, maxlen)))
    return b"".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), rng.integers(0, maxlen)))


def rand_int(rng):
    if rng.integers(0, 3) == 0:
        return INT_EDGES[int(rng.integers(0, len(INT_EDGES)))]
    return int(rng.integers(-2 ** 63, 2 ** 63 - 1))


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def hexes(a) -> list[str]:
    return [x.tobytes().hex() for x in a]


def client_keys(oracle_lib, rng, n_keys=5):
    privs, keys = [], np.zeros((n_keys, 64), np.uint8)
    for k in range(n_keys):
        d = int.from_bytes(rng.bytes(32), "big") % (N_ORDER - 1) + 1
        privs.append(d.to_bytes(32, "big"))
        assert oracle_lib.oracle_p256_pubkey(privs[-1], keys[k].ctypes.data) == 1
    return privs, keys


def signed(oracle_lib, rng, preimages, privs, keys, fmt):
    """Sign each preimage with a random client key and carry that key in fmt;
    corrupt about a third: a flipped r, another client's key, or -- compressed
    -- the wrong-parity prefix; under X||Y the third kind negates y instead
    (the same point the wrong prefix decodes to).
    Returns sigs (n, 64), the key column (n, stride), hashes (n, 32)."""
    sigs, col, hs = [], [], []
    for pre in preimages:
        h = hashlib.sha256(pre).digest()
        key = int(rng.integers(0, len(privs)))
        sig = np.zeros(64, np.uint8)
        while not oracle_lib.oracle_ecdsa_p256_sign(h, privs[key], rng.bytes(32), sig.ctypes.data):
            pass
        sig = sig.tobytes()
        c = int(rng.integers(0, 9))
        xy = keys[key].tobytes()
        if c == 0:
            sig = bytes([sig[0] ^ 1]) + sig[1:]
        elif c == 1:
            xy = keys[(key + 1) % len(privs)].tobytes()
        wire = wc.encode_one(xy, fmt)
        if c == 2:
            if fmt == KEY_SEC1_COMPRESSED:
                wire = wc.encode_one(xy, fmt, wrong_parity=True)
            else:
                y = int.from_bytes(xy[32:], "big")
                wire = wc.encode_one(xy[:32] + (wc.P - y).to_bytes(32, "big"), fmt)
        sigs.append(sig)
        col.append(wire)
        hs.append(h)
    n = len(preimages)
    return (np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64).copy(),
            np.frombuffer(b"".join(col), np.uint8).reshape(n, wc.STRIDE[fmt]).copy(),
            np.frombuffer(b"".join(hs), np.uint8).reshape(n, 32).copy())


def requests_case(oracle_lib, n, fmt):
    rng = np.random.default_rng(7000 + 10 * n + fmt)
    privs, keys = client_keys(oracle_lib, rng)
    reqs = [(rand_int(rng), rand_str(rng), rand_str(rng, 30), 0 if rng.integers(0, 4) else rand_int(rng))
            for _ in range(n)]
    pre = [gojson.request(*r) for r in reqs]
    S, K, H = signed(oracle_lib, rng, pre, privs, keys, fmt)
    assigned = np.array([rand_int(rng) for _ in range(n)], np.int64)
    return reqs, pre, S, K, H, assigned


def replies_case(oracle_lib, n, fmt):
    rng = np.random.default_rng(8000 + 10 * n + fmt)
    privs, keys = client_keys(oracle_lib, rng)
    reps = [(rand_int(rng), rand_int(rng), rand_str(rng), b"node%d" % int(rng.integers(0, 4)),
             [b"Executed", rand_str(rng, 40)][int(rng.integers(0, 2))]) for _ in range(n)]
    pre = [gojson.reply(*r) for r in reps]
    S, K, H = signed(oracle_lib, rng, pre, privs, keys, fmt)
    return reps, pre, S, K, H


def check_requests(v, oracle_lib, n, fmt):
    reqs, pre, S, K, H, assigned = requests_case(oracle_lib, n, fmt)
    want = wc.expect(oracle_lib, H, S, K, fmt)
    dg, ok, cons = v.flush_requests_wirekey(RequestColumns(reqs), S, K, fmt, assigned)
    assert hexes(dg) == [sha(p) for p in pre]
    assert ok.tolist() == want.tolist()
    assert hexes(cons) == [sha(gojson.request(r[0], r[1], r[2], int(a))) for r, a in zip(reqs, assigned)]
    if n >= 67:
        assert ok.any() and not ok.all()
    d2, s2, c2 = v.flush_requests_wirekey(RequestColumns(reqs), S, K, fmt, digests=False)
    assert d2 is None and c2 is None and s2.tolist() == want.tolist()


def check_replies(v, oracle_lib, n, fmt):
    reps, pre, S, K, H = replies_case(oracle_lib, n, fmt)
    want = wc.expect(oracle_lib, H, S, K, fmt)
    dg, ok = v.flush_replies_wirekey(ReplyColumns(reps), S, K, fmt)
    assert hexes(dg) == [sha(p) for p in pre]
    assert ok.tolist() == want.tolist()
    if n >= 67:
        assert ok.any() and not ok.all()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [3, 67, 700])
def test_flush_requests_wirekey_vs_oracle(ver, oracle_lib, n, fmt):
    check_requests(ver, oracle_lib, n, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [3, 67, 700])
def test_flush_replies_wirekey_vs_oracle(ver, oracle_lib, n, fmt):
    check_replies(ver, oracle_lib, n, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_logical_devices(oracle_lib, monkeypatch, fmt):
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    with Verifier(device_mask=1) as v:
        assert v.device_count() == 2
        check_requests(v, oracle_lib, 700, fmt)
        check_replies(v, oracle_lib, 700, fmt)


def test_digests_only_empty_and_bad_arguments(ver, oracle_lib):
    reqs, pre, S, K, H, _ = requests_case(oracle_lib, 67, KEY_SEC1_COMPRESSED)
    cols = RequestColumns(reqs)
    dg, ok, cons = ver.flush_requests_wirekey(cols)  # no signatures wanted: digests alone
    assert ok is None and cons is None and hexes(dg) == [sha(p) for p in pre]
    dg, ok, _ = ver.flush_requests_wirekey(RequestColumns([]), np.zeros((0, 64), np.uint8), np.zeros((0, 33), np.uint8),
                                           KEY_SEC1_COMPRESSED)
    assert len(dg) == 0 and len(ok) == 0
    L, bm, out = ver._L, np.zeros(16, np.uint8), np.zeros((67, 32), np.uint8)
    # an unknown format; a bitmap wanted without keys
    assert L.pbftv_flush_requests_wirekey(ver._h, 67, *cols.args(), S.ctypes.data, K.ctypes.data, 7, None,
                                          out.ctypes.data, bm.ctypes.data, None) == PBFTV_EINVAL
    assert L.pbftv_flush_requests_wirekey(ver._h, 67, *cols.args(), S.ctypes.data, None, KEY_SEC1_COMPRESSED, None,
                                          out.ctypes.data, bm.ctypes.data, None) == PBFTV_EINVAL
    reps, _, S2, K2, _ = replies_case(oracle_lib, 3, KEY_XY)
    rc = ReplyColumns(reps)
    assert L.pbftv_flush_replies_wirekey(ver._h, 3, *rc.args(), S2.ctypes.data, K2.ctypes.data, -1, out.ctypes.data,
                                         bm.ctypes.data) == PBFTV_EINVAL
    assert L.pbftv_flush_replies_wirekey(ver._h, 3, *rc.args(), None, K2.ctypes.data, KEY_XY, out.ctypes.data,
                                         bm.ctypes.data) == PBFTV_EINVAL
