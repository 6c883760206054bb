"""Signing on the GPU through the library: pbftv_register_signing_keys, the
sign batches (host and _dev forms, r||s and DER) and pbftv_sign_replies,
every signature compared byte for byte with tests/rfc6979_model.py and then
verified by the library's own verifies and flushes under the matching public
keys."""
from __future__ import annotations

import numpy as np
import pytest

import msgpath_cases as mc
import rfc6979_model as model
import sign_cases as sc
from oracle import der as oder
from simple_pbft_amd import DerColumn, Verifier
from simple_pbft_amd.pbftv import PBFTV_EINVAL, PBFTV_ENOSIGNKEYS, PBFTV_OK, PbftvError, ReplyColumns

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4096]
NKEYS = 5
BIG = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ver():
    """the five signing keys and, as verify keys, their public halves"""
    ds = sc.keypool(NKEYS)
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).all()
        assert v.register_keys(sc.pubkeys(ds)).all()
        yield v


def raw_bitmap(v, hashes, kidx):
    """the host form with its bitmap bytes as written (padding bits included)"""
    n = len(hashes)
    sig = np.full((n, 64), 0xEE, np.uint8)
    bm = np.full((n + 7) // 8 + 8, 0xFF, np.uint8)
    rc = v._L.pbftv_ecdsa_p256_sign_batch(v._h, hashes.ctypes.data, kidx.ctypes.data, n, sig.ctypes.data,
                                          bm.ctypes.data)
    assert rc == PBFTV_OK
    return sig, bm


@pytest.mark.parametrize("n", SIZES)
def test_sign_batch_matches_the_model_and_verifies(ver, n):
    hashes, kidx, want = sc.batch(n, NKEYS)
    assert n < 63 or len(set(kidx.tolist())) == NKEYS  # every key, in mixed order
    sig, bm = raw_bitmap(ver, hashes, kidx)
    assert (sig == want).all(), np.nonzero((sig != want).any(axis=1))[0]
    nb = (n + 7) // 8
    bits = np.unpackbits(bm[:nb], bitorder="little")
    assert bits[:n].all() and not bits[n:].any()  # ok everywhere, padding bits zero
    assert (bm[nb:] == 0xFF).all()                # nothing written past the bitmap
    assert ver.verify_batch(hashes, sig, kidx).all()
    # without the bitmap: the same rows
    sig2 = np.zeros_like(sig)
    assert ver._L.pbftv_ecdsa_p256_sign_batch(ver._h, hashes.ctypes.data, kidx.ctypes.data, n, sig2.ctypes.data,
                                              None) == PBFTV_OK
    assert (sig2 == want).all()


def test_bad_rows_are_zero_and_leave_their_neighbours_alone():
    """An index past the key set, and keys d = 0 and d = n: 64 zero bytes and a
    0 bit, never an error; every other row is as without them."""
    ds = list(sc.keypool(3)) + [0, sc.N]
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).tolist() == [True, True, True, False, False]
        n = 200
        hashes, kidx, want = sc.batch(n, 3)
        kidx, want = kidx.copy(), want.copy()
        bad = {0: 3, 17: 4, 63: 5, 64: BIG, 130: 3, 199: 1 << 31}
        for i, j in bad.items():
            kidx[i] = j
            want[i] = 0
        sig, ok = v.sign_batch(hashes, kidx)
        assert (sig == want).all()
        assert ok.tolist() == [i not in bad for i in range(n)]
        der, ln = v.sign_der_batch(hashes, kidx)
        assert [int(x) == 0 for x in ln] == [i in bad for i in range(n)]
        assert not der[list(bad)].any()


def test_no_signing_keys_n_zero_and_null_pointers(ver):
    L = ver._L
    h, k = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint32)
    sig, bm = np.zeros((4, 64), np.uint8), np.zeros(8, np.uint8)
    der, ln = np.zeros((4, 72), np.uint8), np.zeros(4, np.uint32)
    hp, kp, sp, bp, dp, lp = (a.ctypes.data for a in (h, k, sig, bm, der, ln))
    with Verifier(device_mask=1) as fresh:
        f = fresh._h
        assert L.pbftv_ecdsa_p256_sign_batch(f, hp, kp, 4, sp, bp) == PBFTV_ENOSIGNKEYS
        assert L.pbftv_ecdsa_p256_sign_der_batch(f, hp, kp, 4, dp, lp) == PBFTV_ENOSIGNKEYS
        dh, dk, ds = fresh.to_device(0, h), fresh.to_device(0, k), fresh.alloc(0, 4 * 72 + 64)
        assert L.pbftv_ecdsa_p256_sign_batch_dev(f, 0, dh.ptr, dk.ptr, 4, ds.ptr, None, None) == PBFTV_ENOSIGNKEYS
        cols = ReplyColumns(mc.layout_batch("reply", 4))
        assert L.pbftv_sign_replies(f, 4, *cols.args(), kp, None, sp, bp) == PBFTV_ENOSIGNKEYS
        assert L.pbftv_ecdsa_p256_sign_batch(f, hp, kp, 0, sp, bp) == PBFTV_OK  # n = 0 asks for nothing
        for b in (dh, dk, ds):
            b.free()
    c = ver._h
    sig[:] = 0xEE
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, kp, 0, sp, bp) == PBFTV_OK and (sig == 0xEE).all()
    assert L.pbftv_ecdsa_p256_sign_batch(c, None, None, 0, None, None) == PBFTV_OK
    assert L.pbftv_ecdsa_p256_sign_der_batch(c, hp, kp, 0, dp, lp) == PBFTV_OK
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, kp, 1 << 32, sp, bp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_der_batch(c, hp, kp, 1 << 32, dp, lp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_batch(None, hp, kp, 4, sp, bp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_batch(c, None, kp, 4, sp, bp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, None, 4, sp, bp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, kp, 4, None, bp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_der_batch(c, hp, kp, 4, None, lp) == PBFTV_EINVAL
    assert L.pbftv_ecdsa_p256_sign_der_batch(c, hp, kp, 4, dp, None) == PBFTV_EINVAL
    assert L.pbftv_register_signing_keys(c, None, 3, None) == PBFTV_EINVAL
    assert L.pbftv_register_signing_keys(None, hp, 1, None) == PBFTV_EINVAL
    dh, dk, ds = ver.to_device(0, h), ver.to_device(0, k), ver.alloc(0, 4 * 72 + 64)
    dl = ver.alloc(0, 64)
    try:
        dev = L.pbftv_ecdsa_p256_sign_batch_dev
        assert dev(c, 0, dh.ptr, dk.ptr, 0, ds.ptr, None, None) == PBFTV_OK
        assert dev(c, 0, None, dk.ptr, 4, ds.ptr, None, None) == PBFTV_EINVAL
        assert dev(c, 0, dh.ptr, None, 4, ds.ptr, None, None) == PBFTV_EINVAL
        assert dev(c, 0, dh.ptr, dk.ptr, 4, None, None, None) == PBFTV_EINVAL
        assert dev(c, 0, dh.ptr + 8, dk.ptr, 4, ds.ptr, None, None) == PBFTV_EINVAL  # misaligned hashes
        assert dev(c, 0, dh.ptr, dk.ptr, 4, ds.ptr + 8, None, None) == PBFTV_EINVAL  # misaligned signatures
        assert dev(c, 0, dh.ptr, dk.ptr, 1 << 32, ds.ptr, None, None) == PBFTV_EINVAL
        assert dev(c, 7, dh.ptr, dk.ptr, 4, ds.ptr, None, None) == PBFTV_EINVAL
        dder = L.pbftv_ecdsa_p256_sign_der_batch_dev
        assert dder(c, 0, dh.ptr, dk.ptr, 4, ds.ptr, None, None) == PBFTV_EINVAL
        assert dder(c, 0, dh.ptr, dk.ptr, 4, ds.ptr + 8, dl.ptr, None) == PBFTV_EINVAL
        ver.sync(0)
    finally:
        for b in (dh, dk, ds, dl):
            b.free()
    cols = ReplyColumns(mc.layout_batch("reply", 4))
    assert L.pbftv_sign_replies(c, 4, *cols.args(), None, None, sp, bp) == PBFTV_EINVAL
    assert L.pbftv_sign_replies(c, 4, *cols.args(), kp, None, None, bp) == PBFTV_EINVAL
    assert L.pbftv_sign_replies(c, 0, *cols.args(), kp, None, sp, bp) == PBFTV_OK


def _sign_then_verify_dev(v, n, stream):
    """sign, then verify on the same stream with no host synchronisation in between"""
    hashes, kidx, want = sc.batch(n, NKEYS)
    nb = (n + 7) // 8
    dh, dk = v.to_device(0, hashes), v.to_device(0, kidx)
    dsig = v.to_device(0, np.full(64 * n + 64, 0xEE, np.uint8))
    dok = v.to_device(0, np.full(nb + 8, 0xFF, np.uint8))
    dbm = v.to_device(0, np.zeros(nb + 8, np.uint8))
    try:
        v.sign_batch_dev(0, dh.ptr, dk.ptr, n, dsig.ptr, dok.ptr, stream=stream)
        v.verify_batch_dev(0, dh.ptr, dsig.ptr, dk.ptr, n, dbm.ptr, stream=stream)
        if stream is None:
            v.sync(0)
        else:
            v.stream_wait(0, stream)
        sig, ok, bm = dsig.to_host(), dok.to_host(), dbm.to_host()
    finally:
        for b in (dh, dk, dsig, dok, dbm):
            b.free()
    assert (sig[:64 * n].reshape(n, 64) == want).all() and (sig[64 * n:] == 0xEE).all()
    for raw in (ok, bm):
        bits = np.unpackbits(raw[:nb], bitorder="little")
        assert bits[:n].all() and not bits[n:].any()
    assert (ok[nb:] == 0xFF).all()


@pytest.mark.parametrize("n", [257, 4096])
def test_dev_form_on_a_library_stream_feeds_the_verify(ver, n, monkeypatch):
    monkeypatch.setenv("PBFTV_WAVE_MAX", "0")  # the verify behind the signer is the lane path's
    st = ver.stream_create(0)
    try:
        _sign_then_verify_dev(ver, n, st)
    finally:
        ver.stream_destroy(0, st)


def test_dev_form_on_the_context_stream(ver, monkeypatch):
    monkeypatch.setenv("PBFTV_WAVE_MAX", "0")
    _sign_then_verify_dev(ver, 300, None)


def test_reregistration_gives_the_new_keys_signatures(ver):
    """A second key set replaces the first; the verify key set and
    pbftv_table_config are what they were before any signing call."""
    n = 130
    cfg = ver.table_config()
    old, new = sc.keypool(NKEYS), sc.keypool(NKEYS, seed=99)
    assert set(old).isdisjoint(new)
    hashes, kidx, want_old = sc.batch(n, NKEYS)
    want_new = np.frombuffer(b"".join(model.sign_bytes(hashes[i].tobytes(), new[kidx[i]]) for i in range(min(n, 96))),
                             np.uint8).reshape(-1, 64)[np.arange(n) % 96]
    try:
        assert ver.register_signing_keys(sc.col(new)).all()
        sig, ok = ver.sign_batch(hashes, kidx)
        assert ok.all() and (sig == want_new).all() and not (sig == want_old).all(axis=1).any()
        assert not ver.verify_batch(hashes, sig, kidx).any()  # the verify keys are still the old public keys
        # fewer keys than before: an index the old set had is now out of range
        assert ver.register_signing_keys(sc.col(new[:2])).all()
        sig2, ok2 = ver.sign_batch(hashes, kidx)
        assert ok2.tolist() == (kidx < 2).tolist()
        assert (sig2[kidx < 2] == want_new[kidx < 2]).all() and not sig2[kidx >= 2].any()
    finally:
        assert ver.register_signing_keys(sc.col(old)).all()
    sig, ok = ver.sign_batch(hashes, kidx)
    assert ok.all() and (sig == want_old).all()
    assert ver.verify_batch(hashes, sig, kidx).all()
    assert ver.table_config() == cfg


def _der_inputs():
    """the searched (hash, key) pairs -- zero top bytes, top bits, the shortest
    and longest encodings -- among ordinary rows, each pair's key a key of its own"""
    fx = sc.der_fixture()
    ds = list(sc.keypool(NKEYS)) + [int(c["d"], 16) for c in fx]
    hashes, kidx, want = sc.batch(257, NKEYS)
    hashes, kidx, want = hashes.copy(), kidx.copy(), want.copy()
    at = [3 + 23 * j for j in range(len(fx))]
    for j, (i, c) in enumerate(zip(at, fx)):
        hashes[i] = np.frombuffer(bytes.fromhex(c["hash"]), np.uint8)
        kidx[i] = NKEYS + j
        want[i] = np.frombuffer(model.sign_bytes(bytes.fromhex(c["hash"]), ds[NKEYS + j]), np.uint8)
    return ds, hashes, kidx, want, at, fx


def test_der_form_parses_back_with_the_models_lengths():
    ds, hashes, kidx, want, at, fx = _der_inputs()
    n = len(hashes)
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).all()
        assert v.register_keys(sc.pubkeys(ds)).all()
        der, ln = v.sign_der_batch(hashes, kidx)
        encs = [sc.der_expected(want[i]) for i in range(n)]
        assert ln.tolist() == [len(e) for e in encs]
        assert [int(ln[i]) for i in at] == [c["der_len"] for c in fx]
        assert {68, 72} <= set(ln.tolist())
        for i in range(n):
            assert der[i, :ln[i]].tobytes() == encs[i] and not der[i, ln[i]:].any(), i
            assert oder.to_rs(der[i, :ln[i]].tobytes()) == want[i].tobytes()
        # the slots as a DER column: the library's own parser and verify take them
        col = DerColumn(blob=der.reshape(-1), off=(72 * np.arange(n)).astype(np.uint64), length=ln.astype(np.uint32))
        assert v.verify_der_batch(hashes, col, kidx).all()
        # _dev form: the same slots and lengths, nothing past them
        dh, dk = v.to_device(0, hashes), v.to_device(0, kidx)
        dd = v.to_device(0, np.full(72 * n + 64, 0xEE, np.uint8))
        dl = v.to_device(0, np.full(n + 4, 0xEEEEEEEE, np.uint32))
        try:
            v.sign_der_batch_dev(0, dh.ptr, dk.ptr, n, dd.ptr, dl.ptr)
            v.sync(0)
            got, gl = dd.to_host(), dl.to_host(dtype=np.uint32)
        finally:
            for b in (dh, dk, dd, dl):
                b.free()
        assert (got[:72 * n].reshape(n, 72) == der).all() and (got[72 * n:] == 0xEE).all()
        assert (gl[:n] == ln).all() and (gl[n:] == 0xEEEEEEEE).all()


_REPLY_WANT = {}


def reply_want(digests, kidx):
    """the model's signatures over the reply digests, computed once for all layouts"""
    key = (digests.tobytes(), kidx.tobytes())
    if key not in _REPLY_WANT:
        ds = sc.keypool(NKEYS)
        _REPLY_WANT[key] = np.frombuffer(
            b"".join(model.sign_bytes(digests[i].tobytes(), ds[kidx[i]]) for i in range(len(kidx))),
            np.uint8).reshape(-1, 64)
    return _REPLY_WANT[key]


@pytest.mark.parametrize("how", ["packed"] + list(mc.LAYOUTS))
def test_sign_replies(ver, how):
    """Digests equal pbftv_digest_reply_batch, signatures equal the model over
    those digests, pbftv_flush_replies[_der] accepts them all -- with the string
    columns' freedoms (shared bytes, any order, gaps, zero-length strings)."""
    n = 257
    packed = ReplyColumns(mc.layout_batch("reply", n))
    cols = packed if how == "packed" else mc.relayout(packed, how)
    kidx = (np.arange(n) * 3 % NKEYS).astype(np.uint32)
    want_d = ver.digest_reply_batch(packed)
    dg, sig, ok = ver.sign_replies(cols, kidx)
    assert (dg == want_d).all() and ok.all()
    want = reply_want(want_d, kidx)
    assert (sig == want).all(), np.nonzero((sig != want).any(axis=1))[0]
    fd, fok = ver.flush_replies(cols, sig, kidx)
    assert (fd == want_d).all() and fok.all()
    dg2, der, ln = ver.sign_replies_der(cols, kidx)
    assert (dg2 == want_d).all()
    for i in range(n):
        assert der[i, :ln[i]].tobytes() == sc.der_expected(want[i]), i
    col = DerColumn(blob=der.reshape(-1), off=(72 * np.arange(n)).astype(np.uint64), length=ln.astype(np.uint32))
    fd, fok = ver.flush_replies_der(cols, col, kidx)
    assert (fd == want_d).all() and fok.all()
    # without the digests: the same signatures
    none, sig3, ok3 = ver.sign_replies(cols, kidx, digests=False)
    assert none is None and ok3.all() and (sig3 == want).all()


def test_timing_id_7_counts_launches_and_resets(ver):
    hashes, kidx, _ = sc.batch(65, NKEYS)
    ver.set_kernel_timing(True)
    try:
        ver.reset_kernel_times()
        assert ver.sign_kernel_time_ms(0, 0) == (0.0, 0)
        ver.sign_batch(hashes, kidx)
        ver.sign_batch(hashes, kidx)
        for stage in (1, 2, 3):
            ms, cnt = ver.sign_kernel_time_ms(0, stage)
            assert cnt == 2 and ms > 0
        assert ver.sign_kernel_time_ms(0, 4) == (0.0, 0)
        ms, cnt = ver.sign_kernel_time_ms(0, 0)
        assert cnt == 6 and ms > 0
        ver.sign_der_batch(hashes, kidx)
        assert ver.sign_kernel_time_ms(0, 4)[1] == 1 and ver.sign_kernel_time_ms(0, 0)[1] == 10
        # the ids 0..5 accessor still refuses 6 and 7, and a stage past 4 is refused here
        for k in (6, 7):
            with pytest.raises(PbftvError) as ei:
                ver.kernel_time_ms(0, k)
            assert ei.value.code == PBFTV_EINVAL
        with pytest.raises(PbftvError) as ei:
            ver.sign_kernel_time_ms(0, 5)
        assert ei.value.code == PBFTV_EINVAL
        ver.reset_kernel_times()
        assert ver.sign_kernel_time_ms(0, 0) == (0.0, 0)
    finally:
        ver.set_kernel_timing(False)
    ver.sign_batch(hashes, kidx)
    assert ver.sign_kernel_time_ms(0, 0) == (0.0, 0)  # timing off: nothing recorded


# ---------------------------------------------------------------- seam hashes through the public calls
def test_seam_hashes_and_end_keys_through_the_public_calls():
    """H1_SEAM x D_ENDS -- the hash at 0, 1, n - 1, n, n + 1 and 2^256 - 1 under
    the keys 1, 2, n - 2 and n - 1 -- among ordinary rows, through sign_batch,
    sign_der_batch and their _dev forms: the model's bytes, and the library's
    own verify accepts them under the matching public keys."""
    import sign_stage_cases as ssc
    ds = list(sc.D_ENDS) + list(sc.keypool(NKEYS))
    seam = sc.drbg_cases()[:len(sc.H1_SEAM) * len(sc.D_ENDS)]
    bh, bk, bw = sc.batch(65 - len(seam), NKEYS)
    hashes = np.concatenate([sc.col([h for _, h in seam]), bh])
    kidx = np.concatenate([np.array([sc.D_ENDS.index(d) for d, _ in seam], np.uint32), bk + len(sc.D_ENDS)])
    want = np.concatenate([ssc.chain_expected()[:len(seam)], bw])
    n = len(kidx)
    encs = [sc.der_expected(want[i]) for i in range(n)]
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(sc.col(ds)).all()
        assert v.register_keys(sc.pubkeys(ds)).all()
        sig, bm = raw_bitmap(v, hashes, kidx)
        assert (sig == want).all(), np.nonzero((sig != want).any(axis=1))[0]
        nb = (n + 7) // 8
        bits = np.unpackbits(bm[:nb], bitorder="little")
        assert bits[:n].all() and not bits[n:].any() and (bm[nb:] == 0xFF).all()
        assert v.verify_batch(hashes, sig, kidx).all()
        der, ln = v.sign_der_batch(hashes, kidx)
        for i in range(n):
            assert ln[i] == len(encs[i]) and der[i, :ln[i]].tobytes() == encs[i] and not der[i, ln[i]:].any(), i
        col = DerColumn(blob=der.reshape(-1), off=(72 * np.arange(n)).astype(np.uint64), length=ln.astype(np.uint32))
        assert v.verify_der_batch(hashes, col, kidx).all()
        dh, dk = v.to_device(0, hashes), v.to_device(0, kidx)
        dsig = v.to_device(0, np.full(64 * n + 64, 0xEE, np.uint8))
        dok = v.to_device(0, np.full(nb + 8, 0xFF, np.uint8))
        dd = v.to_device(0, np.full(72 * n + 64, 0xEE, np.uint8))
        dl = v.to_device(0, np.full(n + 4, 0xEEEEEEEE, np.uint32))
        try:
            v.sign_batch_dev(0, dh.ptr, dk.ptr, n, dsig.ptr, dok.ptr)
            v.sign_der_batch_dev(0, dh.ptr, dk.ptr, n, dd.ptr, dl.ptr)
            v.sync(0)
            gs, go, gd, gl = dsig.to_host(), dok.to_host(), dd.to_host(), dl.to_host(dtype=np.uint32)
        finally:
            for b in (dh, dk, dsig, dok, dd, dl):
                b.free()
        assert (gs[:64 * n].reshape(n, 64) == want).all() and (gs[64 * n:] == 0xEE).all()
        assert (go[:nb] == bm[:nb]).all() and (go[nb:] == 0xFF).all()
        assert (gd[:72 * n].reshape(n, 72) == der).all() and (gd[72 * n:] == 0xEE).all()
        assert (gl[:n] == ln).all() and (gl[n:] == 0xEEEEEEEE).all()


# ---------------------------------------------------------------- two logical devices
@pytest.fixture
def two_devices(monkeypatch):
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    v = Verifier()
    assert v.device_count() == 2 and v.device_id(0) == v.device_id(1)
    assert v.register_signing_keys(sc.col(sc.keypool(NKEYS))).all()
    yield v
    v.close()


SHARD_ALIGN = 512  # pbftv_api.cpp kShardAlign: a host form's shards begin at multiples of it


def _seam(n, ndev=2):
    per = -(-n // ndev)
    return -(-per // SHARD_ALIGN) * SHARD_ALIGN


def raw_sign_calls(v, hashes, cols, kidx, rkidx):
    """Every host form of the signer with its outputs poisoned first and slack past
    each: name -> the arrays as written."""
    L, c, n = v._L, v._h, len(kidx)
    nb = (n + 7) // 8
    hp, kp, rp = hashes.ctypes.data, kidx.ctypes.data, rkidx.ctypes.data
    out = {}

    def bufs():
        return (np.full((n + 1, 64), 0xEE, np.uint8), np.full(nb + 8, 0xFF, np.uint8),
                np.full((n + 1, 72), 0xEE, np.uint8), np.full(n + 4, 0xEEEEEEEE, np.uint32),
                np.full((n + 1, 32), 0xA5, np.uint8))

    sig, bm, der, ln, dg = bufs()
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, kp, n, sig.ctypes.data, bm.ctypes.data) == PBFTV_OK
    out["sign_batch"] = (sig, bm)
    sig, bm, der, ln, dg = bufs()
    assert L.pbftv_ecdsa_p256_sign_batch(c, hp, kp, n, sig.ctypes.data, None) == PBFTV_OK
    out["sign_batch, no bitmap"] = (sig,)
    assert L.pbftv_ecdsa_p256_sign_der_batch(c, hp, kp, n, der.ctypes.data, ln.ctypes.data) == PBFTV_OK
    out["sign_der_batch"] = (der, ln)
    sig, bm, der, ln, dg = bufs()
    assert L.pbftv_sign_replies(c, n, *cols.args(), rp, dg.ctypes.data, sig.ctypes.data, bm.ctypes.data) == PBFTV_OK
    out["sign_replies"] = (dg, sig, bm)
    sig, bm, der, ln, dg = bufs()
    assert L.pbftv_sign_replies(c, n, *cols.args(), rp, None, sig.ctypes.data, bm.ctypes.data) == PBFTV_OK
    out["sign_replies, no digests"] = (sig, bm)
    assert L.pbftv_sign_replies_der(c, n, *cols.args(), rp, dg.ctypes.data, der.ctypes.data,
                                    ln.ctypes.data) == PBFTV_OK
    out["sign_replies_der"] = (dg, der, ln)
    return out


@pytest.mark.parametrize("n", [513, 1031, 2049])
def test_two_devices_give_one_devices_signatures(ver, two_devices, n):
    """The sign host forms sharded over two logical devices: every output equal to
    the one-device call's byte for byte, the first 96 rows equal to the model,
    unsigned rows at the ends and on both sides of the shard seam, exact bits
    there, untouched poison past every output -- and a smaller key set reaches
    both shards."""
    seam = _seam(n)
    assert 0 < seam < n
    bad = sorted({0, 511, 512, n - 1, seam - 1, seam} | ({seam + 9} if seam + 9 < n else set()))
    hashes, kidx, want = sc.batch(n, NKEYS)
    kidx, want = kidx.copy(), want.copy()
    cols = ReplyColumns(mc.layout_batch("reply", n))
    rkidx = (np.arange(n) * 3 % NKEYS).astype(np.uint32)
    for j, i in enumerate(bad):
        kidx[i] = rkidx[i] = (NKEYS, BIG, 1 << 31)[j % 3]
        want[i] = 0
    ok = np.ones(n, bool)
    ok[bad] = False
    nb = (n + 7) // 8
    want_bm = np.packbits(ok, bitorder="little")  # padding bits zero
    cfg = two_devices.table_config()
    one = raw_sign_calls(ver, hashes, cols, kidx, rkidx)
    two = raw_sign_calls(two_devices, hashes, cols, kidx, rkidx)
    assert one.keys() == two.keys()
    for name in one:
        for a, b in zip(one[name], two[name]):
            assert np.array_equal(a, b), name
    # ... and "equal" is not "equally wrong": rows, bits and poison of the two-device outputs on their own
    sig, bm = two["sign_batch"]
    assert (sig[:96] == want[:96]).all() and (sig[:n] == want).all() and (sig[n] == 0xEE).all()
    assert (bm[:nb] == want_bm).all() and (bm[nb:] == 0xFF).all()
    assert (two["sign_batch, no bitmap"][0][:n] == want).all() and (two["sign_batch, no bitmap"][0][n] == 0xEE).all()
    der, ln = two["sign_der_batch"]
    for i in list(range(96)) + bad:
        enc = sc.der_expected(want[i]) if ok[i] else b""
        assert ln[i] == len(enc) and der[i, :len(enc)].tobytes() == enc and not der[i, len(enc):].any(), i
    assert ((ln[:n] == 0) == ~ok).all() and (der[n] == 0xEE).all() and (ln[n:] == 0xEEEEEEEE).all()
    dg, rsig, rbm = two["sign_replies"]
    want_d = ver.digest_reply_batch(cols)
    assert (dg[:n] == want_d).all() and (dg[n] == 0xA5).all()
    rwant = reply_want(want_d[:96], np.where(ok[:96], rkidx[:96], 0).astype(np.uint32)).copy()
    rwant[~ok[:96]] = 0
    assert (rsig[:96] == rwant).all() and not rsig[:n][~ok].any() and (rsig[n] == 0xEE).all()
    assert (rbm[:nb] == want_bm).all() and (rbm[nb:] == 0xFF).all()
    fd, fok = ver.flush_replies(cols, rsig[:n], np.where(ok, rkidx, 0).astype(np.uint32))
    assert (fok == ok).all()  # every signed reply, past the first 96 too, verifies under its key
    nsig, nbm = two["sign_replies, no digests"]
    assert np.array_equal(nsig, rsig) and np.array_equal(nbm, rbm)
    dg2, rder, rln = two["sign_replies_der"]
    assert (dg2[:n] == want_d).all() and (dg2[n] == 0xA5).all()
    for i in list(range(96)) + bad:
        enc = sc.der_expected(rwant[i]) if ok[i] else b""  # (a row past the first 96 is here because it is unsigned)
        assert rln[i] == len(enc) and rder[i, :len(enc)].tobytes() == enc and not rder[i, len(enc):].any(), i
    assert ((rln[:n] == 0) == ~ok).all() and (rder[n] == 0xEE).all() and (rln[n:] == 0xEEEEEEEE).all()
    # a smaller key set, registered on both devices: an index it no longer has is unsigned on both shards
    try:
        assert two_devices.register_signing_keys(sc.col(sc.keypool(NKEYS)[:2])).all()
        sig2, ok2 = two_devices.sign_batch(hashes, kidx)
        keep = ok & (kidx < 2)
        for shard in (slice(0, seam), slice(seam, n)):  # (n = 513: the second shard is one unsigned row)
            assert ok[shard].sum() < 16 or (keep[shard].any() and (~keep & ok)[shard].any())
        assert (ok2 == keep).all() and (sig2[keep] == want[keep]).all() and not sig2[~keep].any()
        der2, ln2 = two_devices.sign_der_batch(hashes, kidx)
        assert ((ln2 == 0) == ~keep).all() and not der2[~keep].any()
    finally:
        assert two_devices.register_signing_keys(sc.col(sc.keypool(NKEYS))).all()
    sig3, ok3 = two_devices.sign_batch(hashes, kidx)
    assert (ok3 == ok).all() and (sig3 == want).all()
    assert two_devices.table_config() == cfg

