"""pbftv_ecdsa_p256_verify_pubkey_batch (host and _dev forms): signatures under
keys that were never registered, each carrying its own key, bit for bit
against the oracle.  The vectors are those of tests/test_varbase_cpu.py (golden
with their keys, conftest.crafted_exceptional(), the ladder / G-part / key
cases of tests/varbase_cases.py), tiled to the sizes at which the kernel's
paths change: below / at / above a wave and a block, a ragged last byte, and
several grid-stride rounds (PBFTV_VARBASE_LANES=256)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import varbase_cases as vc
from simple_pbft_amd import Verifier
from simple_pbft_amd.pbftv import PBFTV_OK, PbftvError

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4097]
PBFTV_EINVAL, PBFTV_ENOKEYS = -1, -5
K_VARBASE = 5


@pytest.fixture(scope="module")
def vectors(oracle_lib):
    return vc.all_vectors(oracle_lib)


@pytest.fixture(scope="module")
def ver():
    """one context for the module; pbftv_register_keys is never called on it"""
    with Verifier(device_mask=1) as v:
        yield v


def tiled(vectors, n):
    idx = np.arange(n) % len(vectors[0])
    return tuple(np.ascontiguousarray(a[idx]) for a in vectors)


def host_raw(v, h, s, p):
    """the host form through the C ABI: the bitmap's ceil(n/8) bytes, after
    checking that nothing past them was written"""
    n, nb = len(h), (len(h) + 7) // 8
    bm = np.full(nb + 4, 0xFF, np.uint8)
    rc = v._L.pbftv_ecdsa_p256_verify_pubkey_batch(v._h, h.ctypes.data, s.ctypes.data, p.ctypes.data, n,
                                                   bm.ctypes.data)
    assert rc == PBFTV_OK
    assert (bm[nb:] == 0xFF).all()
    return bm[:nb]


def dev_raw(v, dev, h, s, p, stream=None):
    """the _dev form on `stream` (None: the context stream), likewise"""
    n, nb = len(h), (len(h) + 7) // 8
    bufs = [v.to_device(dev, h), v.to_device(dev, s), v.to_device(dev, p), v.to_device(dev, np.full(nb + 8, 0xFF, np.uint8))]
    try:
        v.verify_pubkey_batch_dev(dev, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, bufs[3].ptr, stream=stream)
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


@pytest.mark.parametrize("n", SIZES)
def test_sizes_host_and_dev(ver, vectors, n):
    h, s, p, want = tiled(vectors, n)
    check_bitmap(host_raw(ver, h, s, p), want)
    check_bitmap(dev_raw(ver, 0, h, s, p), want)
    assert (ver.verify_pubkey_batch(h, s, p) == want).all()


def test_several_rounds_per_lane(ver, vectors, monkeypatch):
    """256 resident lanes: one block walks 4097 signatures in 17 rounds,
    rebuilding its lanes' tables each round; the last round is one lane."""
    monkeypatch.setenv("PBFTV_VARBASE_LANES", "256")
    h, s, p, want = tiled(vectors, 4097)
    check_bitmap(host_raw(ver, h, s, p), want)
    check_bitmap(dev_raw(ver, 0, h, s, p), want)
    monkeypatch.setenv("PBFTV_VARBASE_LANES", "1024")  # four blocks, a ragged fifth round
    check_bitmap(dev_raw(ver, 0, h, s, p), want)


def test_needs_and_touches_no_registration(vectors):
    h, s, p, want = tiled(vectors, 300)
    with Verifier(device_mask=1) as v:
        assert (v.verify_pubkey_batch(h, s, p) == want).all()
        assert v.table_config()[:2] == (0, 0)  # no registered geometry appeared
        with pytest.raises(PbftvError) as e:
            v.verify_batch(h, s, np.zeros(300, np.uint32))
        assert e.value.code == PBFTV_ENOKEYS
        # empty and oversized batches
        bm = np.full(4, 0xFF, np.uint8)
        L = v._L
        assert L.pbftv_ecdsa_p256_verify_pubkey_batch(v._h, h.ctypes.data, s.ctypes.data, p.ctypes.data, 0,
                                                      bm.ctypes.data) == PBFTV_OK
        assert L.pbftv_ecdsa_p256_verify_pubkey_batch(v._h, None, None, None, 0, None) == PBFTV_OK
        assert L.pbftv_ecdsa_p256_verify_pubkey_batch_dev(v._h, 0, None, None, None, 0, None, None) == PBFTV_OK
        assert (bm == 0xFF).all()
        assert L.pbftv_ecdsa_p256_verify_pubkey_batch(v._h, h.ctypes.data, s.ctypes.data, p.ctypes.data, 1 << 32,
                                                      bm.ctypes.data) == PBFTV_EINVAL
        assert L.pbftv_ecdsa_p256_verify_pubkey_batch_dev(v._h, 0, h.ctypes.data, s.ctypes.data, p.ctypes.data,
                                                          1 << 32, bm.ctypes.data, None) == PBFTV_EINVAL


def test_against_the_registered_path(oracle_lib):
    """12 registered keys: the verify that carries keys[kidx[i]] with signature
    i gives the registered verify's bits, both the oracle's, and leaves the
    registered set as it was."""
    keys, h, s, kidx, p, bad = vc.random_signed(oracle_lib, 12, 342, seed=905, corrupt=0.01, corrupt_keys=False)
    keys, h, s, kidx, p, bad = keys, h[:4096], s[:4096], kidx[:4096], p[:4096], bad[:4096]
    assert (p == keys[kidx]).all() and bad.sum() >= 30
    want = vc.oracle_expect_keyed(oracle_lib, h, s, keys, kidx)
    assert want[~bad].all() and not want[bad].any()
    with Verifier(device_mask=1) as v:
        assert v.register_keys(keys).all()
        cfg = v.table_config()
        reg = v.verify_batch(h, s, kidx)
        pub = v.verify_pubkey_batch(h, s, p)
        assert v.table_config() == cfg
        reg2 = v.verify_batch(h, s, kidx)
    assert (reg == want).all() and (reg2 == want).all()
    assert (pub == want).all(), np.nonzero(pub != want)[0][:8]


def test_caller_stream(ver, vectors):
    h, s, p, want = tiled(vectors, 1000)
    st = ver.stream_create(0)
    try:
        check_bitmap(dev_raw(ver, 0, h, s, p, stream=st), want)
        check_bitmap(dev_raw(ver, 0, h[:65], s[:65], p[:65], stream=st), want[:65])
    finally:
        ver.stream_destroy(0, st)


@pytest.mark.parametrize("n", [2049, 5000])
def test_two_logical_devices(vectors, monkeypatch, n):
    """PBFTV_ALIAS_DEVICES=2: two logical devices on GPU 0, contiguous shards
    (the second one's bitmap lands at its byte offset), one shared G table."""
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    h, s, p, want = tiled(vectors, n)
    with Verifier(device_mask=1) as v:
        assert v.device_count() == 2
        check_bitmap(host_raw(v, h, s, p), want)
        check_bitmap(dev_raw(v, 1, h[:257], s[:257], p[:257]), want[:257])


def test_kernel_timing_id_5(ver, vectors):
    h, s, p, want = tiled(vectors, 257)
    ver.set_kernel_timing(True)
    try:
        ver.reset_kernel_times()
        assert (ver.verify_pubkey_batch(h, s, p) == want).all()
        ms, launches = ver.kernel_time_ms(0, K_VARBASE)
        assert launches >= 1 and ms > 0.0
        with pytest.raises(PbftvError) as e:
            ver.kernel_time_ms(0, K_VARBASE + 1)
        assert e.value.code == PBFTV_EINVAL
    finally:
        ver.set_kernel_timing(False)
