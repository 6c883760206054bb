"""The carried-key verify swept at its seams, on the GPU: tests/carried_cases.py's
combined set (chosen-scalar signatures under keys nobody holds the private
scalar of -- ladder digits at every position, G-comb digits and built-in
doublings / cancellations at windows 0, 1, 15 and the carry-only 17th, keys
with edge coordinates, a sweep of compressed X near 0, near p and at limb
boundaries) through pbftv_ecdsa_p256_verify_pubkey_batch and
pbftv_ecdsa_p256_verify_wirekey_batch in all three key formats, host and _dev
forms, in natural order and in one seeded permutation (so that rerun lanes,
rejected keys and plain lanes share waves both ways), with several rounds per
lane, at ragged lengths of the 33-byte column, and once through a flush.
Every expected bit is the oracle's, under the key Python's decode yields.

What the GPU cannot show: the accept bitmap does not say whether a compressed
key WITHOUT a point was rejected by the decode or only by the signature check
that followed; that is pinned in tests/test_carried_cases.py, where the CPU
build of the same limb code returns the decode's verdict, and likewise whether
the exact rerun ran."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import carried_cases as cc
import wirekey_cases as wc
from oracle import gojson
from simple_pbft_amd import KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY, Verifier
from simple_pbft_amd.pbftv import PBFTV_OK, ReplyColumns

pytestmark = pytest.mark.gpu

FORMATS = [KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY]


@pytest.fixture(scope="module")
def ver():
    """one context for the module; pbftv_register_keys is never called on it"""
    with Verifier(device_mask=1) as v:
        yield v


@pytest.fixture(scope="module")
def combined(oracle_lib):
    return cc.combined(oracle_lib)


@pytest.fixture(scope="module")
def wired(oracle_lib, combined):
    """(order, fmt) -> hashes, sigs, keys in fmt, expected bits"""
    out = {}
    for order in ("natural", "permuted"):
        h, s, xy, want, _ = cc.ordered(combined, order)
        for fmt in FORMATS:
            keys, w = cc.wire(oracle_lib, h, s, xy, fmt)
            assert (w == want).all() and w.any() and not w.all()
            out[order, fmt] = (h, s, keys, w)
    return out


def check_bitmap(raw, want, names=None):
    n = len(want)
    got = np.unpackbits(raw, bitorder="little")
    bad = np.nonzero(got[:n].astype(bool) != want)[0]
    assert not len(bad), [names[i] if names else int(i) for i in bad[:6]]
    assert not got[n:].any(), "padding bits must be zero"


def pubkey_host(v, h, s, p):
    n, nb = len(h), (len(h) + 7) // 8
    bm = np.full(nb + 4, 0xFF, np.uint8)
    assert v._L.pbftv_ecdsa_p256_verify_pubkey_batch(v._h, h.ctypes.data, s.ctypes.data, p.ctypes.data, n,
                                                     bm.ctypes.data) == PBFTV_OK
    assert (bm[nb:] == 0xFF).all()
    return bm[:nb]


def wirekey_host(v, h, s, k, fmt):
    n, nb = len(h), (len(h) + 7) // 8
    bm = np.full(nb + 4, 0xFF, np.uint8)
    assert v._L.pbftv_ecdsa_p256_verify_wirekey_batch(v._h, h.ctypes.data, s.ctypes.data, k.ctypes.data, fmt, n,
                                                      bm.ctypes.data) == PBFTV_OK
    assert (bm[nb:] == 0xFF).all()
    return bm[:nb]


def dev_raw(v, h, s, k, fmt=None):
    """the _dev forms (fmt None: pubkey_batch_dev); the key column's buffer
    ends with its last key, the bitmap's is guarded past ceil(n/8) bytes"""
    n, nb = len(h), (len(h) + 7) // 8
    bufs = [v.to_device(0, h), v.to_device(0, s), v.to_device(0, k), v.to_device(0, np.full(nb + 8, 0xFF, np.uint8))]
    try:
        if fmt is None:
            v.verify_pubkey_batch_dev(0, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, bufs[3].ptr)
        else:
            v.verify_wirekey_batch_dev(0, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, fmt, n, bufs[3].ptr)
        v.sync(0)
        raw = bufs[3].to_host()
    finally:
        for b in bufs:
            b.free()
    assert (raw[nb:] == 0xFF).all()
    return raw[:nb]


def names_in(combined, order):
    idx = np.arange(len(combined["want"])) if order == "natural" else combined["perm"]
    return [combined["names"][i] for i in idx]


@pytest.mark.parametrize("order", ["natural", "permuted"])
def test_pubkey_batch(ver, combined, wired, order):
    h, s, xy, want = wired[order, KEY_XY]
    names = names_in(combined, order)
    check_bitmap(pubkey_host(ver, h, s, xy), want, names)
    check_bitmap(dev_raw(ver, h, s, xy), want, names)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("order", ["natural", "permuted"])
def test_wirekey_batch(ver, combined, wired, order, fmt):
    h, s, k, want = wired[order, fmt]
    names = names_in(combined, order)
    check_bitmap(wirekey_host(ver, h, s, k, fmt), want, names)
    check_bitmap(dev_raw(ver, h, s, k, fmt), want, names)


def test_several_rounds_per_lane(ver, combined, wired, monkeypatch):
    """256 resident lanes: one block walks the set in some twenty rounds, each
    lane rebuilding its table 1Q .. 8Q per round, and the exact rerun re-reads
    the table of the round it runs in"""
    monkeypatch.setenv("PBFTV_VARBASE_LANES", "256")
    names = names_in(combined, "natural")
    h, s, xy, want = wired["natural", KEY_XY]
    check_bitmap(dev_raw(ver, h, s, xy), want, names)
    h, s, k, want = wired["natural", KEY_SEC1_COMPRESSED]
    check_bitmap(wirekey_host(ver, h, s, k, KEY_SEC1_COMPRESSED), want, names)


def test_sec1_family_at_ragged_lengths(ver, oracle_lib):
    """the compressed sweep alone, at its own length and cut so that the
    33-byte column ends 1, 2 and 3 bytes into a word; the key buffer ends with
    the last key"""
    h, s, xy, want, names, _, _ = cc.family(oracle_lib, "sec1")
    k, w = cc.wire(oracle_lib, h, s, xy, KEY_SEC1_COMPRESSED)
    assert (w == want).all()
    lengths = [len(h)] + [max(m for m in range(len(h) - 4, len(h) + 1) if m % 4 == res) for res in (1, 2, 3)]
    assert {33 * m % 4 for m in lengths} >= {1, 2, 3}
    for m in sorted(set(lengths)):
        check_bitmap(dev_raw(ver, h[:m], s[:m], k[:m], KEY_SEC1_COMPRESSED), want[:m], names)
    check_bitmap(wirekey_host(ver, h, s, k, KEY_SEC1_COMPRESSED), want, names)


def test_flush_replies_carries_the_families(ver, oracle_lib):
    """pbftv_flush_replies_wirekey with the key-shape and G-part families'
    (r||s, key) pairs as the client signatures.  The flush hashes the message
    itself, so e is SHA-256 of the reply and not the family's chosen e: u2 =
    r / s stays the chosen ladder scalar under the chosen key, u1 becomes
    whatever the digest makes it, and the oracle (under that digest) rejects
    every such pair.  For accepted bits among them, every reply in five is
    signed honestly under one of the keys Q = d G with the oracle's signer."""
    rows = [cc.family(oracle_lib, f) for f in ("keyshape", "gpart")]
    S = np.concatenate([r[1] for r in rows])
    XY = np.concatenate([r[2] for r in rows])
    rng = np.random.default_rng(20268)
    reps = [(int(rng.integers(0, 9)), int(rng.integers(-2 ** 63, 2 ** 63 - 1)), b"client%d" % i,
             b"node%d" % int(rng.integers(0, 4)), [b"Executed", rng.bytes(int(rng.integers(0, 40)))][i % 2])
            for i in range(len(S))]
    pre = [gojson.reply(*r) for r in reps]
    H = np.frombuffer(b"".join(hashlib.sha256(p).digest() for p in pre), np.uint8).reshape(-1, 32).copy()
    S, XY = S.copy(), XY.copy()
    DK = cc.dlog_keys()
    for i in range(0, len(S), 5):
        _, q, d = DK[(i // 5) % len(DK)]
        while not oracle_lib.oracle_ecdsa_p256_sign(H[i].ctypes.data, d.to_bytes(32, "big"), rng.bytes(32),
                                                    S[i].ctypes.data):
            pass
        XY[i] = np.frombuffer(wc.xy_bytes(*q), np.uint8)
    for fmt in (KEY_SEC1_COMPRESSED, KEY_XY):
        keys, want = cc.wire(oracle_lib, H, S, XY, fmt)
        assert want[::5].all() and want.sum() == len(want[::5])
        dg, ok = ver.flush_replies_wirekey(ReplyColumns(reps), S, keys, fmt)
        assert [x.tobytes() for x in dg] == [hashlib.sha256(p).digest() for p in pre]
        assert ok.tolist() == want.tolist()
