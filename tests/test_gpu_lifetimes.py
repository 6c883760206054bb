"""What a caller does to its buffers between batches.

pbftv_dev_free promises that a block returns to the pool only after the work
queued so far on the context's streams has passed (include/pbftv.h, "device
memory / stream plumbing"); the list behind it is host/pending_frees.h, whose
logic tests/cpp/test_pending_frees.cpp checks on the host.  Here, on the GPU:

  a. a buffer freed while DEPTH batches that use it are still queued on a
     library stream, the same size allocated again at once and overwritten:
     the new block is another one and every batch computed from the old one;
  b. the same with the batches on the context's own stream and on a stream the
     caller made itself (there pbftv_dev_free waits on the host);
  c. 50 free / allocate cycles under queued work leave no pending free and
     create no event after the fifth cycle;
  d. pbftv_close with frees pending and work queued;
  e. pinned blocks: the reuse cache, its "at most twice the size" rule, the
     1 GiB cap, a host-buffer verify from reused blocks;
  f. one batch of every user of the device's shared scratch, alternating over
     the context's stream, a library stream and a caller's own with no host
     synchronisation in between and kernel timing on: every output exact, the
     launch counts of timing ids 0..7 as enqueued, then pbftv_close with event
     pairs nobody collected (host/scratch_order.h, host/kernel_timers.h).

Inputs as in test_gpu_stream_queues.py: 32,768 distinct signatures over 10
keys, 1 % corrupted, tiled to batches of 262,144; the reference is the
construction's expected bits.  Every in-flight case first times one untouched
pass of the same DEPTH batches (the batch time is that pass / DEPTH) and FAILS,
saying so, unless the GPU was still busy for at least two batch times after the
free, the allocation and the overwrite: otherwise it would prove nothing.

Observed on an MI355X (DEPTH = 32, five in-flight cases): batch time
0.281-0.310 ms (an untouched pass of 32 batches 9.0-9.9 ms); pbftv_dev_free
0.006-0.015 ms, the allocation 0.009-0.011 ms, the overwrite 0.034-0.099 ms;
the library stream was then busy for another 8.3-8.8 ms = 28.5-29.7 batch
times (2 are required).  With the batches on the context's stream the
overwrite itself waited 8.7 ms; with them on the caller's own stream
pbftv_dev_free waited 8.7 ms and the stream wait after it took 0.02 ms.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

from conftest import fixture_arrays
from test_gpu_keys_devices import _foreign_stream, ctypes_void
from test_gpu_stream_queues import make_pool, tiled

pytestmark = pytest.mark.gpu

N_BIG, DEPTH = 262144, 32
NB = N_BIG // 8


@pytest.fixture(scope="module")
def pool():
    data = make_pool()
    for a in data:
        a.setflags(write=False)
    return data


class Rig:
    """One context with the keys registered, hashes and signatures resident,
    DEPTH bitmaps and a library stream."""

    def __init__(self, pool):
        from simple_pbft_amd import Verifier
        pub, H, S, K, ok = pool
        self.v = v = Verifier(device_mask=1)
        assert v.register_keys(pub).all()
        self.dh, self.ds = v.to_device(0, tiled(H, N_BIG)), v.to_device(0, tiled(S, N_BIG))
        self.K = tiled(K, N_BIG)
        self.want = np.packbits(tiled(ok, N_BIG), bitorder="little")
        self.maps = [v.alloc(0, NB) for _ in range(DEPTH)]
        self.lib_stream = v.stream_create(0)

    def counters(self):
        c = self.v.lib_counters(0)
        assert c["held_events"] + c["spare_events"] == c["events_created"], c
        return c

    def enqueue(self, dk, bitmap, stream):
        self.v.verify_batch_dev(0, self.dh.ptr, self.ds.ptr, dk.ptr, N_BIG, bitmap.ptr, stream=stream)

    def wait(self, stream):
        if stream is None:
            self.v.sync(0)
        else:
            self.v.stream_wait(0, stream)

    def wrong(self, bitmaps):
        return [j for j, b in enumerate(bitmaps) if not (b.to_host() == self.want).all()]

    def close(self):
        self.v.close()


@pytest.fixture(scope="module")
def rig(pool):
    r = Rig(pool)
    yield r
    r.close()


def untouched_pass(rig, dk, stream):
    """DEPTH batches, nothing freed: every bitmap right; returns the batch time in s."""
    for b in rig.maps:
        b.zero()
    t0 = time.perf_counter()
    for b in rig.maps:
        rig.enqueue(dk, b, stream)
    rig.wait(stream)
    t = (time.perf_counter() - t0) / DEPTH
    assert rig.wrong(rig.maps) == []
    for b in rig.maps:
        b.zero()
    return t


def ms(seconds):
    return f"{seconds * 1e3:.3f} ms"


def free_in_flight(rig, kind, victim):
    """The common shape of tests a and b.  kind: where the DEPTH batches are
    queued ("library", "context", "foreign"); victim: the buffer freed right
    after the last enqueue ("keys": the key indices every batch reads;
    "bitmap": the last batch's bitmap)."""
    v = rig.v
    hip = None
    if kind == "library":
        stream = rig.lib_stream
    elif kind == "context":
        stream = None
    else:
        hip, stream = _foreign_stream()
    dk = v.to_device(0, rig.K)
    keep = None
    try:
        # one pass to place each stream's scratch, then the timed one
        untouched_pass(rig, dk, stream)
        batch = untouched_pass(rig, dk, stream)
        keep = v.alloc(0, 64)  # (an allocation reaps: nothing is pending from here on)
        assert rig.counters()["pending_frees"] == 0
        for b in rig.maps:
            rig.enqueue(dk, b, stream)
        t_queued = time.perf_counter()
        old = dk if victim == "keys" else rig.maps[-1]
        old_ptr, size = old.ptr, old.nbytes
        old.free()
        t_freed = time.perf_counter()
        new = v.alloc(0, size)
        c = rig.counters()
        t_alloc = time.perf_counter()
        if victim == "keys":
            dk = new
            poison = np.full(N_BIG, 0xFFFFFFF0, np.uint32)  # every key index out of range: all-zero bitmaps
            assert v._L.pbftv_memcpy_h2d(v._h, 0, new.ptr, poison.ctypes.data, poison.nbytes) == 0
        else:
            rig.maps[-1] = new
            assert v._L.pbftv_memset_dev(v._h, 0, new.ptr, 0xFF, size) == 0
        t_copied = time.perf_counter()
        rig.wait(stream)
        t_done = time.perf_counter()
        print(f"[lifetimes {kind}/{victim}] batch {ms(batch)}, free {ms(t_freed - t_queued)}, alloc "
              f"{ms(t_alloc - t_freed)}, overwrite {ms(t_copied - t_alloc)}, wait after it {ms(t_done - t_copied)} "
              f"= {(t_done - t_copied) / batch:.1f} batches; pending frees after the alloc {c['pending_frees']}, "
              f"new block {'the same' if new.ptr == old_ptr else 'another'}")
        if kind == "library":
            busy = t_done - t_copied
            assert busy >= 2 * batch, (f"not in flight: the stream was busy for {ms(busy)} after the overwrite, "
                                       f"less than two batch times of {ms(batch)}")
        elif kind == "context":  # (the overwrite goes through the context's stream: it is the wait)
            busy = t_done - t_alloc
            assert busy >= 2 * batch, (f"not in flight: the stream was busy for {ms(busy)} after the allocation, "
                                       f"less than two batch times of {ms(batch)}")
        else:  # the caller's own stream: the free itself waited for the work, on the host
            assert t_freed - t_queued >= 2 * batch, f"not in flight: pbftv_dev_free took {ms(t_freed - t_queued)}"
            assert t_done - t_copied < batch, f"work left on the caller's stream after the free: {ms(t_done - t_copied)}"
        if kind != "foreign":  # the GPU was busy past the allocation, so the marks had not passed
            assert c["pending_frees"] >= 1 and c["held_events"] >= 2, c
        if c["pending_frees"] >= 1:
            assert new.ptr != old_ptr, "a block whose free is pending was handed out again"
        if victim == "keys":
            assert rig.wrong(rig.maps) == [], "batches queued before the free read the new block"
        else:
            assert rig.wrong(rig.maps[:-1]) == []
            assert (new.to_host() == 0xFF).all(), "the last batch wrote into the new block"
    finally:
        rig.wait(stream)
        if hip is not None:
            hip.hipStreamDestroy(ctypes_void(stream))
        if keep is not None:
            keep.free()
        if dk.ptr:
            dk.free()


def test_free_of_an_input_while_batches_are_queued(rig):
    """a.  The key-index buffer, freed under 32 batches of 262,144 on a library
    stream, re-allocated and filled with out-of-range indices.

    Measured on an MI355X: batch 0.309 ms, free + allocation + overwrite
    0.124 ms, then the stream busy for 8.799 ms = 28.5 batch times; one free
    pending after the allocation, the new block another one."""
    free_in_flight(rig, "library", "keys")


def test_free_of_an_output_while_batches_are_queued(rig):
    """a, second variant.  The last batch's bitmap; the new block is filled with
    0xFF and must still hold it when the stream has drained (the freed pointer
    is not read).

    Measured on an MI355X: batch 0.282 ms, free + allocation + overwrite
    0.050 ms, then the stream busy for 8.365 ms = 29.7 batch times."""
    free_in_flight(rig, "library", "bitmap")


@pytest.mark.parametrize("kind", ["context", "library", "foreign"])
def test_marks_on_every_stream_kind(rig, kind):
    """b.  The key-index buffer freed under 32 batches on each kind of stream.

    Measured on an MI355X: context stream: batch 0.310 ms, the overwrite (a
    copy on that stream) waited 8.723 ms; library stream: batch 0.281 ms, busy
    for 8.319 ms after the overwrite; caller's own stream: batch 0.296 ms,
    pbftv_dev_free waited 8.743 ms on the host, the stream wait after it took
    0.022 ms (less than one batch time is required)."""
    free_in_flight(rig, kind, "keys")


def test_free_cycles_do_not_grow(rig):
    """c.  50 cycles of: a batch on the library stream, its bitmap freed and
    allocated again, the stream waited for, one more allocation and free.

    Measured on an MI355X: 4 events created after cycle 1, 4 after cycle 50."""
    v, st = rig.v, rig.lib_stream
    dk = v.to_device(0, rig.K)
    bm = v.alloc(0, NB)
    created = {}
    last = None
    try:
        for cycle in range(1, 51):
            rig.enqueue(dk, bm, st)
            bm.free()
            bm = v.alloc(0, NB)
            v.stream_wait(0, st)
            x = v.alloc(0, NB)
            x.free()
            created[cycle] = rig.counters()["events_created"]
        v.sync(0)
        v.stream_wait(0, st)
        last = v.alloc(0, NB)  # (an allocation reaps; every stream has been waited for)
        c = rig.counters()
        print(f"[lifetimes cycles] events created after cycle 1 / 5 / 50: {created[1]} / {created[5]} / {created[50]}; {c}")
        assert c["pending_frees"] == 0 and c["held_events"] == 0
        assert c["spare_events"] == c["events_created"]
        assert created[50] == created[5]
        bm.zero()
        rig.enqueue(dk, bm, st)
        v.stream_wait(0, st)
        assert rig.wrong([bm]) == []
    finally:
        v.stream_wait(0, st)
        for b in (dk, bm, last):
            if b is not None:
                b.free()


def test_close_with_pending_frees_and_queued_work(pool, ecdsa_fixtures, monkeypatch):
    """d.  pbftv_close with DEPTH batches queued on a library stream and every
    buffer they use already freed (pending); then a fresh context verifies the
    golden vectors."""
    from simple_pbft_amd import Verifier
    monkeypatch.setenv("PBFTV_GBITS", "24")  # small tables: this test is about bookkeeping
    monkeypatch.setenv("PBFTV_QBITS", "16")
    r = Rig(pool)
    try:
        dk = r.v.to_device(0, r.K)
        for b in r.maps:
            r.enqueue(dk, b, r.lib_stream)
        for b in [dk, r.dh, r.ds] + r.maps:
            b.free()
        c = r.counters()
        print(f"[lifetimes close] {c}")
        assert c["pending_frees"] >= 1
    finally:
        r.close()  # (returns nothing: a failure inside it would abort or hang here)
    assert r.v.handle is None
    keys, hashes, sigs, kidx, expect = fixture_arrays(ecdsa_fixtures)
    with Verifier(device_mask=1) as v:
        v.register_keys(keys)
        assert (v.verify_batch(hashes, sigs, kidx) == expect).all()


def test_every_scratch_user_across_three_streams_with_timing_on(oracle_lib, monkeypatch):
    """f.  One batch of every user of the device's shared scratch -- registered
    and carried-key (SEC1 compressed) verifies, both with DER signatures too, a
    sign and a sign-DER batch, a SHA-256 length order -- enqueued with no host
    synchronisation in between, alternating over the context's stream, a
    library stream and a stream the caller made; 65 items each (a wave plus
    one: a ragged last bitmap byte), one signature per verify corrupted, every
    batch on the lane path, kernel timing on.  After one synchronisation every
    output equals the oracle's or the RFC 6979 model's, and the launch counts
    of ids 0..7, read through the three getters, are what the sequence
    implies.  Then more DER and sign launches, and the context closes with
    their times uncollected."""
    import hashlib

    import msgpath_cases as mc
    import sign_cases as sc
    import wirekey_cases as wk
    from simple_pbft_amd import Verifier
    from simple_pbft_amd.pbftv import KEY_SEC1_COMPRESSED
    monkeypatch.setenv("PBFTV_GBITS", "24")  # small tables: this test is about ordering and bookkeeping
    monkeypatch.setenv("PBFTV_QBITS", "16")
    monkeypatch.setenv("PBFTV_WAVE_MAX", "0")
    n, nkeys, nb = 65, 5, 9
    ds = sc.keypool(nkeys)
    pub = sc.pubkeys(ds)
    hashes, kidx, model_rs = sc.batch(n, nkeys)

    def corrupted(at):  # the model's signatures with one s byte flipped
        s = model_rs.copy()
        s[at, 40] ^= 0x10
        return s

    def oracle_bits(sigs):
        want = np.zeros(nb, np.uint8)
        oracle_lib.oracle_ecdsa_p256_verify_batch(hashes.ctypes.data, sigs.ctypes.data, kidx.ctypes.data, n,
                                                  pub.ctypes.data, nkeys, want.ctypes.data, 4)
        bits = np.unpackbits(want, bitorder="little")[:n].astype(bool)
        assert bits.sum() == n - 1  # exactly the corrupted one fails
        return bits

    def der_column(sigs):
        encs = [sc.der_expected(sigs[i]) for i in range(n)]
        length = np.array([len(e) for e in encs], np.uint32)
        off = (np.cumsum(length) - length).astype(np.uint64)
        return np.frombuffer(b"".join(encs), np.uint8), off, length

    sig_a, sig_b, sig_c, sig_d = corrupted(0), corrupted(63), corrupted(64), corrupted(17)
    want_bits = [oracle_bits(s) for s in (sig_a, sig_b, sig_c, sig_d)]
    carried = wk.encode(pub[kidx], KEY_SEC1_COMPRESSED)
    want_der = [sc.der_expected(model_rs[i]) for i in range(n)]
    msgs = [bytes([i]) * (3 + 7 * i) for i in range(n)]  # 3 .. 451 bytes: one to eight compressions
    m_data, m_off, m_len = Verifier.pack(msgs)
    want_digests = np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), np.uint8).reshape(n, 32)

    v = Verifier(device_mask=1)
    hip, foreign = _foreign_stream()
    try:
        v.set_latency_path_max(0)
        assert v.register_keys(pub).all() and v.register_signing_keys(sc.col(ds)).all()
        lib = v.stream_create(0)
        up = lambda a: v.to_device(0, a, pad=64)
        dh, dk, dkeys = up(hashes), up(kidx), up(carried)
        d_sig_a, d_sig_b = up(sig_a), up(sig_b)
        d_der_c, d_der_d = [up(x) for x in der_column(sig_c)], [up(x) for x in der_column(sig_d)]
        d_bits = [v.alloc(0, 64) for _ in range(4)]
        d_rs, d_ok = v.alloc(0, 64 * n + 64), v.alloc(0, 64)
        d_slots, d_slen = v.alloc(0, 72 * n + 64), v.alloc(0, 4 * n + 64)
        d_msg, d_moff, d_mlen = up(m_data), up(m_off), up(m_len)
        d_order, d_dig = v.alloc(0, 4 * n + 64), v.alloc(0, 32 * n + 64)
        outs = d_bits + [d_rs, d_ok, d_slots, d_slen, d_order, d_dig]

        def sequence():
            v.verify_batch_dev(0, dh.ptr, d_sig_a.ptr, dk.ptr, n, d_bits[0].ptr, stream=None)
            v.verify_wirekey_batch_dev(0, dh.ptr, d_sig_b.ptr, dkeys.ptr, KEY_SEC1_COMPRESSED, n, d_bits[1].ptr,
                                       stream=lib)
            v.verify_der_batch_dev(0, dh.ptr, d_der_c[0].ptr, d_der_c[1].ptr, d_der_c[2].ptr, dk.ptr, n,
                                   d_bits[2].ptr, stream=foreign)
            v.verify_wirekey_der_batch_dev(0, dh.ptr, d_der_d[0].ptr, d_der_d[1].ptr, d_der_d[2].ptr, dkeys.ptr,
                                           KEY_SEC1_COMPRESSED, n, d_bits[3].ptr, stream=None)
            v.sign_batch_dev(0, dh.ptr, dk.ptr, n, d_rs.ptr, d_ok.ptr, stream=lib)
            v.sign_der_batch_dev(0, dh.ptr, dk.ptr, n, d_slots.ptr, d_slen.ptr, stream=foreign)
            v.sha256_order_dev(0, d_mlen.ptr, n, d_order.ptr, stream=None)
            v.sha256_batch_dev(0, d_msg.ptr, d_moff.ptr, d_mlen.ptr, d_order.ptr, n, d_dig.ptr, stream=None)

        def wait_all():
            v.sync(0)
            v.stream_wait(0, lib)
            v.stream_wait(0, foreign)

        # once untimed: tables and scratch are placed (their first use synchronises inside the library)
        sequence()
        wait_all()
        for b in outs:
            b.zero()
        v.set_kernel_timing(True)
        v.reset_kernel_times()
        sequence()
        wait_all()

        for j in range(4):
            got = np.unpackbits(d_bits[j].to_host(nb), bitorder="little")[:n].astype(bool)
            assert (got == want_bits[j]).all(), (j, np.nonzero(got != want_bits[j])[0])
        assert (d_rs.to_host(64 * n).reshape(n, 64) == model_rs).all()
        ok = np.unpackbits(d_ok.to_host(nb), bitorder="little")
        assert ok[:n].all() and not ok[n:].any()
        slots, slen = d_slots.to_host(72 * n).reshape(n, 72), d_slen.to_host(4 * n, dtype=np.uint32)
        for i in range(n):
            assert slen[i] == len(want_der[i]) and slots[i, :slen[i]].tobytes() == want_der[i], i
            assert not slots[i, slen[i]:].any(), i
        order = d_order.to_host(4 * n, dtype=np.uint32).astype(np.int64)
        assert (np.sort(order) == np.arange(n)).all()
        assert (np.diff(mc.sha_blocks(m_len)[order]) <= 0).all()  # most compressions first
        assert (d_dig.to_host(32 * n).reshape(n, 32) == want_digests).all()

        # ids 0..5, the DER id and the sign id, each through its own getter
        counts = [v.kernel_time_ms(0, k)[1] for k in range(6)]
        assert counts == [4, 2, 1, 0, 0, 2], counts  # scalars, comb, sha256, wave, gojson, varbase
        assert v.der_kernel_time_ms(0)[1] == 2
        assert [v.sign_kernel_time_ms(0, s)[1] for s in range(5)] == [7, 2, 2, 2, 1]
        assert all(v.kernel_time_ms(0, k)[0] > 0 for k in (0, 1, 2, 5))
        assert v.der_kernel_time_ms(0)[0] > 0 and v.sign_kernel_time_ms(0, 0)[0] > 0

        # DER and sign launches whose times nobody collects
        v.verify_der_batch_dev(0, dh.ptr, d_der_c[0].ptr, d_der_c[1].ptr, d_der_c[2].ptr, dk.ptr, n, d_bits[2].ptr,
                               stream=lib)
        v.sign_der_batch_dev(0, dh.ptr, dk.ptr, n, d_slots.ptr, d_slen.ptr, stream=foreign)
        wait_all()
    finally:
        v.close()  # (returns nothing: a failure inside it would abort or hang here)
        hip.hipStreamDestroy(ctypes_void(foreign))
    assert v.handle is None


def test_pinned_blocks(pool, monkeypatch):
    """e.  pbftv_host_alloc / pbftv_host_free: the cached block comes back for
    the same size and for half of it, not for less than half; a host-buffer
    verify from reused blocks is exact; past 1 GiB of freed blocks the largest
    leaves first (a block from the cache keeps its contents, a new one does
    not hold them)."""
    from simple_pbft_amd import Verifier
    from simple_pbft_amd.pbftv import PinnedArray
    monkeypatch.setenv("PBFTV_GBITS", "24")  # small tables: this test is about host memory
    monkeypatch.setenv("PBFTV_QBITS", "16")
    pub, H, S, K, ok = pool
    MiB = 1 << 20
    with Verifier(device_mask=1) as v:
        a = PinnedArray(v, (MiB,), np.uint8)
        p = a.ptr
        a.free()
        a = PinnedArray(v, (MiB,), np.uint8)
        assert a.ptr == p, "the cached block did not come back for the same size"
        a.free()
        small = PinnedArray(v, (MiB // 2 - 1,), np.uint8)  # less than half: not that block
        assert small.ptr != p
        half = PinnedArray(v, (MiB // 2,), np.uint8)  # exactly half: at most twice the size asked for
        assert half.ptr == p
        small.free()
        half.free()

        # a verify from reused blocks (first filled with something else)
        assert v.register_keys(pub).all()
        first = [PinnedArray(v, x.shape, x.dtype) for x in (H, S, K)]
        ptrs = [q.ptr for q in first]
        for q in first:
            q.a.view(np.uint8)[...] = 0xA5
            q.free()
        again = [v.pinned(x) for x in (H, S, K)]
        assert sorted(q.ptr for q in again) == sorted(ptrs)
        assert (v.verify_batch(again[0].a, again[1].a, again[2].a) == ok).all()
        for q in again:
            q.free()

        # the cap: 448 MiB then 640 MiB freed, 1,088 MiB in all: the 640 MiB block goes
        big, mid = PinnedArray(v, (640 * MiB,), np.uint8), PinnedArray(v, (448 * MiB,), np.uint8)
        marks = np.arange(0, 448 * MiB, 64 * MiB)
        big.a[marks], mid.a[marks] = 0xB1, 0xC2
        p_mid = mid.ptr
        mid.free()
        big.free()
        mid = PinnedArray(v, (448 * MiB,), np.uint8)
        assert mid.ptr == p_mid and (mid.a[marks] == 0xC2).all(), "the smaller block was not kept"
        big = PinnedArray(v, (640 * MiB,), np.uint8)
        assert not (big.a[marks] == 0xB1).any(), "the largest block was still in the cache past the cap"
        big.free()
        mid.free()
