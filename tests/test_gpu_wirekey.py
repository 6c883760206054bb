"""pbftv_ecdsa_p256_verify_wirekey_batch (host and _dev forms): signatures whose
keys arrive in SEC1 wire form (33 B compressed, 65 B uncompressed) or as X||Y,
bit for bit against the oracle under the key a Python big-integer decode yields
(tests/wirekey_cases.py; a key Python rejects expects a 0 bit).  The vectors
are varbase_cases.all_vectors re-encoded, tiled to the sizes at which the key
kernel's paths change (below / at / above a wave and a block, a ragged last
word of the column), the rejected-encoding set spread through the waves,
several rounds per lane, two logical devices (the shard seam at an odd byte
stride), a caller stream, and the argument checks."""
from __future__ import annotations

import numpy as np
import pytest

import varbase_cases as vc
import wirekey_cases as wc
from simple_pbft_amd import KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY, Verifier, key_bytes
from simple_pbft_amd.pbftv import PBFTV_EINVAL, PBFTV_OK

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 256, 257, 1000]
FORMATS = [KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY]


@pytest.fixture(scope="module")
def vectors(oracle_lib):
    """all_vectors in each format: fmt -> (hashes, sigs, keys (n, stride), expect)"""
    h, s, p, want_xy = vc.all_vectors(oracle_lib)
    out = {}
    for fmt in FORMATS:
        keys = wc.encode(p, fmt)
        want = wc.expect(oracle_lib, h, s, keys, fmt)
        if fmt != KEY_SEC1_COMPRESSED:  # (compressed drops Y: an off-curve key may land on a point)
            assert (want == want_xy).all()
        assert want.any() and not want.all()
        out[fmt] = (h, s, keys, want)
    return out


@pytest.fixture(scope="module")
def ver():
    """one context for the module; pbftv_register_keys is never called on it"""
    with Verifier(device_mask=1) as v:
        yield v


def tiled(vec, n):
    idx = np.arange(n) % len(vec[0])
    return tuple(np.ascontiguousarray(a[idx]) for a in vec)


def host_raw(v, h, s, k, fmt):
    """the host form through the C ABI: the bitmap's ceil(n/8) bytes, after
    checking that nothing past them was written"""
    n, nb = len(h), (len(h) + 7) // 8
    bm = np.full(nb + 4, 0xFF, np.uint8)
    rc = v._L.pbftv_ecdsa_p256_verify_wirekey_batch(v._h, h.ctypes.data, s.ctypes.data, k.ctypes.data, fmt, n,
                                                    bm.ctypes.data)
    assert rc == PBFTV_OK
    assert (bm[nb:] == 0xFF).all()
    return bm[:nb]


def dev_raw(v, dev, h, s, k, fmt, stream=None):
    """the _dev form on `stream` (None: the context stream), likewise; the key
    column's buffer ends with its last key"""
    n, nb = len(h), (len(h) + 7) // 8
    bufs = [v.to_device(dev, h), v.to_device(dev, s), v.to_device(dev, k),
            v.to_device(dev, np.full(nb + 8, 0xFF, np.uint8))]
    try:
        v.verify_wirekey_batch_dev(dev, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, fmt, n, bufs[3].ptr, stream=stream)
        if stream is None:
            v.sync(dev)
        else:
            v.stream_wait(dev, stream)
        raw = bufs[3].to_host()
    finally:
        for b in bufs:
            b.free()
    assert (raw[nb:] == 0xFF).all()
    return raw[:nb]


def check_bitmap(raw, want):
    n = len(want)
    got = np.unpackbits(raw, bitorder="little")
    assert (got[:n].astype(bool) == want).all(), np.nonzero(got[:n].astype(bool) != want)[0][:8]
    assert not got[n:].any(), "padding bits must be zero"


def test_key_bytes():
    assert [key_bytes(f) for f in (KEY_XY, KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, 3, -1)] == [64, 33, 65, 0, 0]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_host_and_dev(ver, vectors, n, fmt):
    h, s, k, want = tiled(vectors[fmt], n)
    check_bitmap(host_raw(ver, h, s, k, fmt), want)
    check_bitmap(dev_raw(ver, 0, h, s, k, fmt), want)
    assert (ver.verify_wirekey_batch(h, s, k, fmt) == want).all()


@pytest.mark.parametrize("fmt", [KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED])
def test_rejected_encodings_among_accepted(ver, oracle_lib, fmt):
    """every third key is one of the rejected-encoding set (and the wrong-parity
    key, which decodes to (x, p - y)), the rest the valid key: each wave holds
    both, and the expected bit is the oracle's under Python's decode"""
    h, s, k, want = wc.spread(oracle_lib, fmt, 300)
    assert want[0] and want.any() and not want.all()
    assert want.reshape(-1, 3)[:, :2].all()  # the valid key between them is accepted
    check_bitmap(host_raw(ver, h, s, k, fmt), want)
    check_bitmap(dev_raw(ver, 0, h, s, k, fmt), want)


def test_wrong_parity_is_the_negated_key(ver, oracle_lib):
    """a signature made under (x, p - y) verifies under the wrong-parity prefix of (x, y) only"""
    h0, s0, xy, _ = wc.rejected_set(oracle_lib)
    x, y = int.from_bytes(xy[:32].tobytes(), "big"), int.from_bytes(xy[32:].tobytes(), "big")
    flipped = wc.encode_one(xy.tobytes(), KEY_SEC1_COMPRESSED, wrong_parity=True)
    assert wc.decode(flipped, KEY_SEC1_COMPRESSED) == (x, wc.P - y)
    keys = np.frombuffer(wc.encode_one(xy.tobytes(), KEY_SEC1_COMPRESSED) + flipped, np.uint8).reshape(2, 33)
    h, s = np.tile(h0, (2, 1)), np.tile(s0, (2, 1))
    want = wc.expect(oracle_lib, h, s, keys, KEY_SEC1_COMPRESSED)
    assert want.tolist() == [True, False]
    assert ver.verify_wirekey_batch(h, s, keys, KEY_SEC1_COMPRESSED).tolist() == [True, False]


def test_several_rounds_per_lane(ver, vectors, monkeypatch):
    """256 resident lanes: one block of k_varbase walks 1000 signatures in four
    rounds behind the key kernel's four blocks"""
    monkeypatch.setenv("PBFTV_VARBASE_LANES", "256")
    h, s, k, want = tiled(vectors[KEY_SEC1_COMPRESSED], 1000)
    check_bitmap(host_raw(ver, h, s, k, KEY_SEC1_COMPRESSED), want)
    check_bitmap(dev_raw(ver, 0, h, s, k, KEY_SEC1_COMPRESSED), want)


@pytest.mark.parametrize("n", [1000, 2049])
def test_two_logical_devices(vectors, monkeypatch, n):
    """PBFTV_ALIAS_DEVICES=2: the second shard's keys start at 33 * lo, an odd
    byte offset of the caller's column, and its bitmap lands at its byte offset"""
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    h, s, k, want = tiled(vectors[KEY_SEC1_COMPRESSED], n)
    with Verifier(device_mask=1) as v:
        assert v.device_count() == 2
        check_bitmap(host_raw(v, h, s, k, KEY_SEC1_COMPRESSED), want)
        check_bitmap(dev_raw(v, 1, h[:257], s[:257], k[:257], KEY_SEC1_COMPRESSED), want[:257])


@pytest.mark.parametrize("fmt", [KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED])
def test_caller_stream(ver, vectors, fmt):
    h, s, k, want = tiled(vectors[fmt], 1000)
    st = ver.stream_create(0)
    try:
        check_bitmap(dev_raw(ver, 0, h, s, k, fmt, stream=st), want)
        check_bitmap(dev_raw(ver, 0, h[:65], s[:65], k[:65], fmt, stream=st), want[:65])
    finally:
        ver.stream_destroy(0, st)


def test_needs_no_registration(vectors):
    """a context that never registered keys: no entry point returns PBFTV_ENOKEYS,
    and no registered geometry appears"""
    with Verifier(device_mask=1) as v:
        for fmt in FORMATS:
            h, s, k, want = tiled(vectors[fmt], 300)
            check_bitmap(host_raw(v, h, s, k, fmt), want)
            check_bitmap(dev_raw(v, 0, h, s, k, fmt), want)
        assert v.table_config()[:2] == (0, 0)


def test_registration_undisturbed(oracle_lib, vectors):
    """registered keys: verify_batch gives the same (the oracle's) bits before
    and after wirekey calls in every format, and the geometry stays"""
    keys, h, s, kidx, p, bad = vc.random_signed(oracle_lib, 6, 100, seed=611, corrupt=0.05, corrupt_keys=False)
    want = vc.oracle_expect_keyed(oracle_lib, h, s, keys, kidx)
    assert want[~bad].all() and not want[bad].any() and bad.any()
    with Verifier(device_mask=1) as v:
        assert v.register_keys(keys).all()
        cfg = v.table_config()
        before = v.verify_batch(h, s, kidx)
        for fmt in FORMATS:
            wire = wc.encode(p, fmt)
            assert (v.verify_wirekey_batch(h, s, wire, fmt) == want).all()
            hh, ss, kk, ww = tiled(vectors[fmt], 257)
            assert (v.verify_wirekey_batch(hh, ss, kk, fmt) == ww).all()
        assert v.table_config() == cfg
        after = v.verify_batch(h, s, kidx)
    assert (before == want).all() and (after == want).all()


def test_bad_arguments(ver, vectors):
    h, s, k, _ = tiled(vectors[KEY_SEC1_COMPRESSED], 64)
    L, ctx = ver._L, ver._h
    bm = np.full(16, 0xFF, np.uint8)
    args = (h.ctypes.data, s.ctypes.data, k.ctypes.data)
    for fmt in (3, -1, 255):  # an unknown format, whatever n
        assert L.pbftv_ecdsa_p256_verify_wirekey_batch(ctx, *args, fmt, 64, bm.ctypes.data) == PBFTV_EINVAL
        assert L.pbftv_ecdsa_p256_verify_wirekey_batch(ctx, *args, fmt, 0, bm.ctypes.data) == PBFTV_EINVAL
        assert L.pbftv_ecdsa_p256_verify_wirekey_batch_dev(ctx, 0, *args, fmt, 64, bm.ctypes.data, None) == PBFTV_EINVAL
    # a null key pointer with n > 0; n = 0 is a no-op; n >= 2^32
    assert L.pbftv_ecdsa_p256_verify_wirekey_batch(ctx, args[0], args[1], None, KEY_SEC1_COMPRESSED, 64,
                                                   bm.ctypes.data) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_verify_wirekey_batch(ctx, None, None, None, KEY_SEC1_COMPRESSED, 0, None) == PBFTV_OK
    assert L.pbftv_ecdsa_p256_verify_wirekey_batch_dev(ctx, 0, None, None, None, KEY_SEC1_UNCOMPRESSED, 0, None,
                                                       None) == PBFTV_OK
    assert L.pbftv_ecdsa_p256_verify_wirekey_batch(ctx, *args, KEY_SEC1_COMPRESSED, 1 << 32,
                                                   bm.ctypes.data) == PBFTV_EINVAL
    assert (bm == 0xFF).all()
    # the _dev form: a null key pointer, and a key column that is not 16-B aligned
    bufs = [ver.to_device(0, h), ver.to_device(0, s), ver.to_device(0, k, pad=64), ver.alloc(0, 64)]
    try:
        ptrs = [b.ptr for b in bufs]
        assert all(p % 16 == 0 for p in ptrs)
        dev = L.pbftv_ecdsa_p256_verify_wirekey_batch_dev
        assert dev(ctx, 0, ptrs[0], ptrs[1], None, KEY_SEC1_COMPRESSED, 64, ptrs[3], None) == PBFTV_EINVAL
        for off in (1, 4, 8):
            assert dev(ctx, 0, ptrs[0], ptrs[1], ptrs[2] + off, KEY_SEC1_COMPRESSED, 8, ptrs[3], None) == PBFTV_EINVAL
        assert dev(ctx, 0, ptrs[0] + 8, ptrs[1], ptrs[2], KEY_SEC1_COMPRESSED, 8, ptrs[3], None) == PBFTV_EINVAL
        assert dev(ctx, 0, ptrs[0], ptrs[1], ptrs[2], KEY_SEC1_COMPRESSED, 1 << 32, ptrs[3], None) == PBFTV_EINVAL
    finally:
        for b in bufs:
            b.free()
