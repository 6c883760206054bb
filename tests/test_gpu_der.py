"""Signatures as ASN.1 DER, parsed on the GPU: pbftv_ecdsa_der_to_rs_batch_dev
(k_der_to_rs), pbftv_ecdsa_p256_verify_der_batch and
pbftv_ecdsa_p256_verify_wirekey_der_batch, host and _dev forms.  The corpus
and its placement are tests/der_cases.py's (valid signatures re-encoded, every
class of rejected encoding, at every offset modulo 16, shuffled, sharing
bytes, truncated encodings followed by the bytes that would complete them, the
last encoding ending the buffer, a 72-byte encoding whose length is claimed as
2^32 - 1); every expectation is oracle/der.py's and the oracle verify's.  The
verifies must also equal the existing r||s calls fed oracle/der.to_rs output."""
from __future__ import annotations

import time

import numpy as np
import pytest

import der_cases as dc
import wirekey_cases as wc
from simple_pbft_amd import KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY, DerColumn, Verifier
from simple_pbft_amd.pbftv import K_ECDSA_DER, K_ECDSA_WAVE, PbftvError, PBFTV_EINVAL, PBFTV_ENOKEYS, PBFTV_OK

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 256, 257, 1000]
BIG = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ver():
    """pbftv_register_keys is never called on this context"""
    with Verifier(device_mask=1) as v:
        yield v


@pytest.fixture(scope="module")
def ver_reg(oracle_lib):
    """the golden keys registered"""
    keys = dc.registered_corpus(oracle_lib)[0]
    with Verifier(device_mask=1) as v:
        v.register_keys(keys)
        yield v


@pytest.fixture(scope="module")
def carried_bits(oracle_lib):
    """fmt -> the carried corpus' expected bits under its keys in that format
    (a compressed key drops Y: an off-curve key may land on a point)"""
    hashes, pubs, corpus = dc.carried_corpus(oracle_lib)
    rows = np.array([c.row for c in corpus])
    rs, ok = dc.expected_rs(corpus)
    out = {}
    for fmt in (KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY):
        out[fmt] = wc.expect(oracle_lib, hashes[rows], rs, wc.encode(pubs[rows], fmt), fmt) & ok
    assert (out[KEY_XY] == dc.carried_batch(oracle_lib, len(corpus))[-1]).all()
    return out


def carried(oracle_lib, carried_bits, n, fmt, claim=None):
    h, pubs, cases, rs, ok, _ = dc.carried_batch(oracle_lib, n, claim)
    bits = carried_bits[fmt][np.arange(n) % len(carried_bits[fmt])].copy()
    if claim is not None and n > 1:
        bits[-1] = False
    return h, wc.encode(pubs, fmt), cases, rs, ok, bits


class Column:
    """a placed DER column on the device; the data buffer ends with the blob"""

    def __init__(self, v, dev, blob, off, ln):
        self.bufs = [v.to_device(dev, blob), v.to_device(dev, off), v.to_device(dev, ln)]
        self.ptrs = [b.ptr for b in self.bufs]

    def free(self):
        for b in self.bufs:
            b.free()


def wait(v, dev, stream):
    if stream is None:
        v.sync(dev)
    else:
        v.stream_wait(dev, stream)


def normalise_dev(v, cases, seed, with_bitmap=True, stream=None, dev=0):
    """pbftv_ecdsa_der_to_rs_batch_dev: (r||s rows, parsed bitmap bytes or None),
    after checking the 0xFF guards behind both outputs"""
    n, nb = len(cases), (len(cases) + 7) // 8
    blob, off, ln = dc.place(cases, seed)
    if (ln != 0).any():
        assert int((off + np.minimum(ln, 72))[ln != 0].max()) == len(blob)
    col = Column(v, dev, blob, off, ln)
    out = v.to_device(dev, np.full(64 * n + 64, 0xFF, np.uint8))
    bm = v.to_device(dev, np.full(nb + 8, 0xFF, np.uint8)) if with_bitmap else None
    try:
        v.der_to_rs_batch_dev(dev, *col.ptrs, n, out.ptr, bm.ptr if bm else None, stream=stream)
        wait(v, dev, stream)
        rs, raw = out.to_host(), bm.to_host() if bm else None
    finally:
        col.free()
        out.free()
        if bm:
            bm.free()
    assert (rs[64 * n:] == 0xFF).all(), "bytes past out_rs were written"
    if raw is not None:
        assert (raw[nb:] == 0xFF).all(), "bytes past the parsed bitmap were written"
        raw = raw[:nb]
    return rs[:64 * n].reshape(n, 64), raw


def check_bitmap(raw, want):
    n = len(want)
    got = np.unpackbits(raw, bitorder="little")
    assert (got[:n].astype(bool) == want).all(), np.nonzero(got[:n].astype(bool) != want)[0][:8]
    assert not got[n:].any(), "padding bits must be zero"


@pytest.mark.parametrize("n", SIZES)
def test_der_to_rs_batch_dev(ver, oracle_lib, n):
    _, _, cases, want_rs, want_ok, bits = dc.registered_batch(oracle_lib, n, claim=BIG)
    if n >= 63:
        assert want_ok.any() and not want_ok.all()
        assert sum(c.valid_class for c in cases) * 2 >= n - 1
    if n == 1000:
        dc.check_corpus(dc.registered_corpus(oracle_lib)[-1], dc.registered_batch(oracle_lib, 1000)[-1])
        assert any(c.claim == BIG for c in cases) and any(c.far for c in cases)
    rs, raw = normalise_dev(ver, cases, seed=n)
    bad = np.nonzero((rs != want_rs).any(axis=1))[0]
    assert len(bad) == 0, [cases[i].name for i in bad[:4]]
    check_bitmap(raw, want_ok)
    rs, raw = normalise_dev(ver, cases, seed=n + 1, with_bitmap=False)
    assert raw is None and (rs == want_rs).all()


def test_der_to_rs_batch_dev_on_a_library_stream(ver, oracle_lib):
    st = ver.stream_create(0)
    try:
        for n in (65, 1000):
            _, _, cases, want_rs, want_ok, _ = dc.carried_batch(oracle_lib, n, claim=BIG)
            rs, raw = normalise_dev(ver, cases, seed=3 * n, stream=st)
            assert (rs == want_rs).all()
            check_bitmap(raw, want_ok)
    finally:
        ver.stream_destroy(0, st)


def der_launches(v, dev=0):
    return v.der_kernel_time_ms(dev)[1]


def host_column(cases, seed, claim_room=0):
    """the column in host memory; claim_room: filler appended so that a claimed
    length of that many bytes stays inside the blob"""
    blob, off, ln = dc.place(cases, seed, tight_end=claim_room == 0)
    if claim_room:
        blob = np.concatenate([blob, np.random.default_rng(seed).integers(1, 256, claim_room, dtype=np.uint8)])
        assert int((off + ln)[ln != 0].max()) <= len(blob)
    return DerColumn(blob=blob, off=off, length=ln)


def verify_der_host_raw(v, h, col, signer, fmt=None):
    n, nb = len(h), (len(h) + 7) // 8
    bm = np.full(nb + 4, 0xFF, np.uint8)
    if fmt is None:
        rc = v._L.pbftv_ecdsa_p256_verify_der_batch(v._h, h.ctypes.data, *col.args(), signer.ctypes.data, n,
                                                    bm.ctypes.data)
    else:
        rc = v._L.pbftv_ecdsa_p256_verify_wirekey_der_batch(v._h, h.ctypes.data, *col.args(), signer.ctypes.data, fmt,
                                                            n, bm.ctypes.data)
    assert rc == PBFTV_OK
    assert (bm[nb:] == 0xFF).all()
    return bm[:nb]


def verify_der_dev_raw(v, dev, h, cases, seed, signer, fmt=None, stream=None):
    n, nb = len(h), (len(h) + 7) // 8
    col = Column(v, dev, *dc.place(cases, seed))
    bufs = [v.to_device(dev, h), v.to_device(dev, signer), v.to_device(dev, np.full(nb + 8, 0xFF, np.uint8))]
    try:
        if fmt is None:
            v.verify_der_batch_dev(dev, bufs[0].ptr, *col.ptrs, bufs[1].ptr, n, bufs[2].ptr, stream=stream)
        else:
            v.verify_wirekey_der_batch_dev(dev, bufs[0].ptr, *col.ptrs, bufs[1].ptr, fmt, n, bufs[2].ptr,
                                           stream=stream)
        wait(v, dev, stream)
        raw = bufs[2].to_host()
    finally:
        col.free()
        for b in bufs:
            b.free()
    assert (raw[nb:] == 0xFF).all()
    return raw[:nb]


@pytest.mark.parametrize("latency_max", [0, 2048])
@pytest.mark.parametrize("n", SIZES)
def test_verify_der_registered(ver_reg, oracle_lib, n, latency_max):
    """latency_max 0: every size takes the lane path and the device normaliser;
    2048 (the default): the host form parses on the host and takes the latency
    path -- no k_der_to_rs launch -- while the _dev form normalises on the device"""
    v = ver_reg
    v.set_latency_path_max(latency_max)
    v.set_kernel_timing(True)
    try:
        h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, n, claim=10000)
        legacy = v.verify_batch(h, rs, kidx)  # the r||s call fed oracle/der.to_rs output
        assert (legacy == bits).all()
        v.reset_kernel_times()
        waves0 = v.kernel_time_ms(0, K_ECDSA_WAVE)[1]
        check_bitmap(verify_der_host_raw(v, h, host_column(cases, n, claim_room=10000), kidx), bits)
        if latency_max == 0:
            assert der_launches(v) == 1 and v.kernel_time_ms(0, K_ECDSA_WAVE)[1] == waves0
        else:
            assert der_launches(v) == 0
        assert (v.verify_der_batch(h, host_column(cases, n + 7, claim_room=10000), kidx) == bits).all()
        v.reset_kernel_times()
        h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, n, claim=BIG)
        check_bitmap(verify_der_dev_raw(v, 0, h, cases, n, kidx), bits)
        assert der_launches(v) == 1
    finally:
        v.set_kernel_timing(False)
        v.set_latency_path_max(2048)


@pytest.mark.parametrize("n", SIZES)
def test_verify_der_wirekey(ver, oracle_lib, carried_bits, n):
    fmt = KEY_SEC1_COMPRESSED
    h, keys, cases, rs, ok, bits = carried(oracle_lib, carried_bits, n, fmt, claim=10000)
    assert (ver.verify_wirekey_batch(h, rs, keys, fmt) == bits).all()
    ver.set_kernel_timing(True)
    try:
        ver.reset_kernel_times()
        check_bitmap(verify_der_host_raw(ver, h, host_column(cases, n, claim_room=10000), keys, fmt), bits)
        assert der_launches(ver) == 1  # (the carried-key verify has no latency path)
    finally:
        ver.set_kernel_timing(False)
    assert (ver.verify_wirekey_der_batch(h, host_column(cases, n + 7, claim_room=10000), keys, fmt) == bits).all()
    h, keys, cases, rs, ok, bits = carried(oracle_lib, carried_bits, n, fmt, claim=BIG)
    check_bitmap(verify_der_dev_raw(ver, 0, h, cases, n, keys, fmt), bits)


@pytest.mark.parametrize("fmt", [KEY_SEC1_UNCOMPRESSED, KEY_XY])
def test_verify_der_wirekey_other_formats(ver, oracle_lib, carried_bits, fmt):
    h, keys, cases, rs, ok, bits = carried(oracle_lib, carried_bits, 257, fmt, claim=BIG)
    assert bits.any() and not bits.all()
    check_bitmap(verify_der_dev_raw(ver, 0, h, cases, 5, keys, fmt), bits)
    assert (ver.verify_wirekey_der_batch(h[:-1], host_column(cases[:-1], 6), keys[:-1], fmt) == bits[:-1]).all()


def test_library_stream_and_context_stream_interleaved(ver_reg, oracle_lib):
    """the device's one r||s scratch is ordered across streams: a stream from
    pbftv_stream_create and the context stream alternate on one device"""
    v = ver_reg
    v.set_latency_path_max(0)
    st = v.stream_create(0)
    try:
        for n, stream in ((1000, st), (257, None), (65, st), (1000, None)):
            h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, n, claim=BIG)
            check_bitmap(verify_der_dev_raw(v, 0, h, cases, n, kidx, stream=stream), bits)
    finally:
        v.stream_destroy(0, st)
        v.set_latency_path_max(2048)


def odd_seam_column(cases, lo):
    """a placement in which the encodings of [lo, n) begin at an odd offset of the blob"""
    for seed in range(64):
        col = host_column(cases, seed)
        used = col.off[lo:][col.len[lo:] != 0]
        if int(used.min()) % 2 == 1:
            return col
    raise AssertionError("no placement with an odd shard seam")


@pytest.mark.parametrize("n", [1001, 2049])
def test_two_logical_devices(oracle_lib, carried_bits, monkeypatch, n):
    """PBFTV_ALIAS_DEVICES=2, n odd: the second shard's span starts at an odd
    byte offset of the caller's blob, and its bitmap lands at its byte offset"""
    monkeypatch.setenv("PBFTV_ALIAS_DEVICES", "2")
    lo = (n + 1) // 2 + 511 & ~511
    keys_reg = dc.registered_corpus(oracle_lib)[0]
    with Verifier(device_mask=1) as v:
        assert v.device_count() == 2
        v.register_keys(keys_reg)
        v.set_latency_path_max(0)
        v.set_kernel_timing(True)
        h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, n)
        check_bitmap(verify_der_host_raw(v, h, odd_seam_column(cases, lo), kidx), bits)
        assert der_launches(v, 0) == 1 and der_launches(v, 1) == 1
        h, keys, cases, rs, ok, bits = carried(oracle_lib, carried_bits, n, KEY_SEC1_COMPRESSED)
        check_bitmap(verify_der_host_raw(v, h, odd_seam_column(cases, lo), keys, KEY_SEC1_COMPRESSED), bits)
        h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, 257, claim=BIG)
        check_bitmap(verify_der_dev_raw(v, 1, h, cases, 1, kidx), bits)


def test_wirekey_form_needs_no_registration_and_disturbs_none(ver, ver_reg, oracle_lib, carried_bits):
    h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, 300)
    col = host_column(cases, 1)
    bm = np.zeros(64, np.uint8)
    # no keys registered: the registered forms say so, the carried-key forms work
    assert ver._L.pbftv_ecdsa_p256_verify_der_batch(ver._h, h.ctypes.data, *col.args(), kidx.ctypes.data, 300,
                                                    bm.ctypes.data) == PBFTV_ENOKEYS
    dcol = Column(ver, 0, col.blob, col.off, col.len)
    bufs = [ver.to_device(0, h), ver.to_device(0, kidx), ver.alloc(0, 64)]
    try:
        assert ver._L.pbftv_ecdsa_p256_verify_der_batch_dev(ver._h, 0, bufs[0].ptr, *dcol.ptrs, bufs[1].ptr, 300,
                                                            bufs[2].ptr, None) == PBFTV_ENOKEYS
    finally:
        dcol.free()
        for b in bufs:
            b.free()
    assert ver.table_config()[:2] == (0, 0)
    hc, keys, ccases, _, _, cbits = carried(oracle_lib, carried_bits, 300, KEY_XY)
    assert (ver.verify_wirekey_der_batch(hc, host_column(ccases, 2), keys, KEY_XY) == cbits).all()
    assert ver.table_config()[:2] == (0, 0)
    # registered keys: the same bits before and after carried-key DER calls, the geometry unchanged
    cfg = ver_reg.table_config()
    ver_reg.set_latency_path_max(0)
    try:
        before = ver_reg.verify_der_batch(h, col, kidx)
        assert (ver_reg.verify_wirekey_der_batch(hc, host_column(ccases, 3), keys, KEY_XY) == cbits).all()
        after = ver_reg.verify_der_batch(h, col, kidx)
    finally:
        ver_reg.set_latency_path_max(2048)
    assert ver_reg.table_config() == cfg
    assert (before == bits).all() and (after == bits).all()


def test_bad_arguments(ver, ver_reg, oracle_lib):
    h, kidx, cases, rs, ok, bits = dc.registered_batch(oracle_lib, 64)
    col = host_column(cases, 9)
    pubs = np.zeros((64, 33), np.uint8)
    L = ver._L
    bm = np.full(16, 0xFF, np.uint8)
    hp, kp, pp, b = h.ctypes.data, kidx.ctypes.data, pubs.ctypes.data, bm.ctypes.data
    blob, off, ln = col.args()
    reg, wk = L.pbftv_ecdsa_p256_verify_der_batch, L.pbftv_ecdsa_p256_verify_wirekey_der_batch
    ctx = ver_reg._h
    # null buffers with n > 0
    assert reg(ctx, None, blob, off, ln, kp, 64, b) == PBFTV_EINVAL
    assert reg(ctx, hp, blob, None, ln, kp, 64, b) == PBFTV_EINVAL
    assert reg(ctx, hp, blob, off, None, kp, 64, b) == PBFTV_EINVAL
    assert reg(ctx, hp, blob, off, ln, None, 64, b) == PBFTV_EINVAL
    assert reg(ctx, hp, blob, off, ln, kp, 64, None) == PBFTV_EINVAL
    assert reg(ctx, hp, None, off, ln, kp, 64, b) == PBFTV_EINVAL  # lengths promise bytes, no blob
    assert reg(None, hp, blob, off, ln, kp, 64, b) == PBFTV_EINVAL
    assert wk(ver._h, hp, blob, off, ln, None, KEY_SEC1_COMPRESSED, 64, b) == PBFTV_EINVAL
    assert wk(ver._h, hp, blob, off, ln, pp, 3, 64, b) == PBFTV_EINVAL
    assert wk(ver._h, hp, blob, off, ln, pp, -1, 0, b) == PBFTV_EINVAL
    # n = 0 writes nothing, whatever the pointers; n = 2^32 touches no buffer
    assert reg(ctx, None, None, None, None, None, 0, None) == PBFTV_OK
    assert reg(ver._h, None, None, None, None, None, 0, None) == PBFTV_OK  # (no keys there either)
    assert wk(ver._h, None, None, None, None, None, KEY_XY, 0, None) == PBFTV_OK
    assert reg(ctx, hp, blob, off, ln, kp, 1 << 32, b) == PBFTV_EINVAL
    assert wk(ver._h, hp, blob, off, ln, pp, KEY_XY, 1 << 32, b) == PBFTV_EINVAL
    assert (bm == 0xFF).all()
    # the _dev forms
    dcol = Column(ver, 0, col.blob, col.off, col.len)
    bufs = [ver.to_device(0, h), ver.to_device(0, kidx), ver.alloc(0, 64 * 64 + 64), ver.alloc(0, 64),
            ver.to_device(0, pubs, pad=64)]
    try:
        dh, dk, drs, dbm, dp = (x.ptr for x in bufs)
        assert drs % 16 == 0
        norm = L.pbftv_ecdsa_der_to_rs_batch_dev
        assert norm(ver._h, 0, *dcol.ptrs, 64, drs + 8, dbm, None) == PBFTV_EINVAL  # misaligned out_rs
        assert norm(ver._h, 0, *dcol.ptrs, 64, drs + 4, None, None) == PBFTV_EINVAL
        assert norm(ver._h, 0, *dcol.ptrs, 64, None, dbm, None) == PBFTV_EINVAL
        assert norm(ver._h, 0, dcol.ptrs[0], None, dcol.ptrs[2], 64, drs, dbm, None) == PBFTV_EINVAL
        assert norm(ver._h, 0, dcol.ptrs[0], dcol.ptrs[1], None, 64, drs, dbm, None) == PBFTV_EINVAL
        assert norm(ver._h, 0, None, None, None, 0, None, None, None) == PBFTV_OK
        assert norm(ver._h, 0, *dcol.ptrs, 1 << 32, drs, dbm, None) == PBFTV_EINVAL
        for dev in (-1, 1, 7):
            assert norm(ver._h, dev, *dcol.ptrs, 64, drs, dbm, None) == PBFTV_EINVAL
            assert L.pbftv_ecdsa_p256_verify_der_batch_dev(ctx, dev, dh, *dcol.ptrs, dk, 64, dbm, None) == PBFTV_EINVAL
            assert L.pbftv_ecdsa_p256_verify_wirekey_der_batch_dev(ver._h, dev, dh, *dcol.ptrs, dp, KEY_XY, 64, dbm,
                                                                   None) == PBFTV_EINVAL
        rdev, wdev = L.pbftv_ecdsa_p256_verify_der_batch_dev, L.pbftv_ecdsa_p256_verify_wirekey_der_batch_dev
        # (ctx is another context on the same GPU: device pointers are the process's)
        assert rdev(ctx, 0, dh + 8, *dcol.ptrs, dk, 64, dbm, None) == PBFTV_EINVAL
        assert rdev(ctx, 0, dh, *dcol.ptrs, None, 64, dbm, None) == PBFTV_EINVAL
        assert rdev(ctx, 0, dh, *dcol.ptrs, dk, 1 << 32, dbm, None) == PBFTV_EINVAL
        assert rdev(ctx, 0, None, None, None, None, None, 0, None, None) == PBFTV_OK
        assert wdev(ver._h, 0, dh, *dcol.ptrs, dp + 4, KEY_SEC1_COMPRESSED, 8, dbm, None) == PBFTV_EINVAL
        assert wdev(ver._h, 0, dh, *dcol.ptrs, dp, 9, 8, dbm, None) == PBFTV_EINVAL
        assert wdev(ver._h, 0, dh, *dcol.ptrs, dp, KEY_XY, 1 << 32, dbm, None) == PBFTV_EINVAL
        assert wdev(ver._h, 0, None, None, None, None, None, KEY_XY, 0, None, None) == PBFTV_OK
    finally:
        dcol.free()
        for x in bufs:
            x.free()


@pytest.mark.parametrize("kind", ["library", "foreign"])
def test_blob_freed_right_after_the_enqueue(kind):
    """The DER blob freed with pbftv_dev_free right after DEPTH batches of
    verify_der_batch_dev were enqueued on a caller stream, the same size
    allocated again and overwritten with 0xFF: every batch still computed from
    the encodings (on a stream the library made, the free is deferred behind
    marks; on the caller's own stream pbftv_dev_free waits on the host)."""
    from test_gpu_keys_devices import _foreign_stream, ctypes_void
    from test_gpu_stream_queues import tiled  # (puts tools/ on the path)
    import synth
    from oracle import der as oder
    N, DEPTH = 262144, 12
    pub, H, S, K, ok = synth.config4(8192, n_keys=10, seed=0xDE5)
    ders = [oder.encode(int.from_bytes(r[:32].tobytes(), "big"), int.from_bytes(r[32:].tobytes(), "big")) for r in S]
    blob1, off1, ln1 = Verifier.pack(ders)
    reps = N // len(ders)
    blob = np.tile(blob1, reps)
    off = (np.tile(off1, reps) + np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(len(blob1)), len(ders)))
    ln = np.tile(ln1, reps)
    want = np.packbits(tiled(ok, N), bitorder="little")
    assert ok.any() and not ok.all()
    hip = None
    with Verifier(device_mask=1) as v:
        assert v.register_keys(pub).all()
        if kind == "library":
            stream = v.stream_create(0)
        else:
            hip, stream = _foreign_stream()
        dh, dk = v.to_device(0, tiled(H, N)), v.to_device(0, tiled(K, N))
        doff, dln = v.to_device(0, off), v.to_device(0, ln)
        dblob = v.to_device(0, blob)
        maps = [v.alloc(0, N // 8) for _ in range(DEPTH)]
        try:
            def enqueue_all():
                for m in maps:
                    v.verify_der_batch_dev(0, dh.ptr, dblob.ptr, doff.ptr, dln.ptr, dk.ptr, N, m.ptr, stream=stream)
            enqueue_all()  # places the scratch
            v.stream_wait(0, stream)
            t0 = time.perf_counter()
            enqueue_all()
            v.stream_wait(0, stream)
            batch = (time.perf_counter() - t0) / DEPTH
            assert all((m.to_host() == want).all() for m in maps)
            for m in maps:
                m.zero()
            enqueue_all()
            t_queued = time.perf_counter()
            old_ptr, size = dblob.ptr, dblob.nbytes
            dblob.free()
            t_freed = time.perf_counter()
            dblob = v.alloc(0, size)
            c = v.lib_counters(0)
            assert v._L.pbftv_memset_dev(v._h, 0, dblob.ptr, 0xFF, size) == 0
            v.stream_wait(0, stream)
            print(f"[der lifetimes {kind}] batch {batch * 1e3:.3f} ms, free {(t_freed - t_queued) * 1e3:.3f} ms, "
                  f"pending frees after the allocation {c['pending_frees']}")
            if kind == "library":
                # the marks of the free had not passed when the allocation looked: the batches were in flight
                # (the 19 MB overwrite is a kernel that shares the GPU with them, so its end proves nothing)
                assert c["pending_frees"] >= 1, "not in flight: the free's marks had passed before the allocation"
                assert dblob.ptr != old_ptr, "a block whose free is pending was handed out again"
            else:
                assert t_freed - t_queued >= 2 * batch, "not in flight: pbftv_dev_free did not wait"
            wrong = [j for j, m in enumerate(maps) if not (m.to_host() == want).all()]
            assert wrong == [], "batches queued before the free read the new block"
        finally:
            v.stream_wait(0, stream)
            if hip is not None:
                hip.hipStreamDestroy(ctypes_void(stream))


def test_timing_id_6_has_its_own_accessor(ver, oracle_lib):
    """PBFTV_K_ECDSA_DER = 6 is read through pbftv_der_kernel_time_ms and reset
    with the other ids; pbftv_kernel_time_ms keeps refusing every id past 5"""
    _, _, cases, _, _, _ = dc.registered_batch(oracle_lib, 65)
    assert K_ECDSA_DER == 6
    ver.set_kernel_timing(True)
    try:
        ver.reset_kernel_times()
        assert ver.der_kernel_time_ms(0) == (0.0, 0)
        normalise_dev(ver, cases, seed=6)
        normalise_dev(ver, cases, seed=7, with_bitmap=False)
        ms, launches = ver.der_kernel_time_ms(0)
        assert launches == 2 and ms > 0.0
        for bad in (K_ECDSA_DER, K_ECDSA_DER + 1, -1):
            with pytest.raises(PbftvError) as e:
                ver.kernel_time_ms(0, bad)
            assert e.value.code == PBFTV_EINVAL
        with pytest.raises(PbftvError) as e:
            ver.der_kernel_time_ms(1)
        assert e.value.code == PBFTV_EINVAL
        ver.reset_kernel_times()
        assert ver.der_kernel_time_ms(0) == (0.0, 0)
    finally:
        ver.set_kernel_timing(False)
