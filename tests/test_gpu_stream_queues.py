"""Streams from pbftv_stream_create hold a hardware queue of their own
(pbftv_api.cpp own_queue_stream), whatever streams the context made before:

  1. independence: a small batch on stream B, enqueued after 16 large batches
     on stream A, finishes long before A does -- on a shared queue it could not
     finish before A (the property bench.py's step overlap depends on);
  2. correctness of interleaved batches on four such streams, at the smallest
     size that reaches each stage variant of the lane path;
  3. more streams than the cap of dedicated queues (Device::kOwnQueues = 8),
     destroyed and created again, then pbftv_close.

PBFTV_STREAM_QUEUE=shared (plain streams, the behaviour before) is read once
per process, so those runs are fresh child processes of this file.

Inputs: 32,768 distinct OpenSSL signatures over 10 keys, 1 % corrupted
(tools/synth.py), signed once per module and tiled for the larger sizes
(duplicates verify the same).  The reference is the construction's expected
bits, tiled the same way.

Observed on an MI355X (test 1, twelve ordered pairs): t_A 4.46-5.34 ms, t_B
0.36-0.64 ms, t_B / t_A 0.080-0.120.  With PBFTV_STREAM_QUEUE=shared, in the
same set-up: 0.997 and 0.998 for the two pairs whose streams shared a hardware
queue (the first and the second stream), 0.080-0.092 for the other ten.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

POOL = 32768
N_KEYS = 10
N_BIG, N_SMALL, DEPTH = 262144, 4096, 16
# (n, the path it is the smallest size for)
SIZES = [(4096, "lane path, no key order, K = 1"), (32768, "key order"), (131072, "K = 2"),
         (262144, "K = 4, block inversion")]
SHIFT = 4096  # stream j reads its inputs SHIFT * j signatures further on: four different bitmaps


def make_pool():
    import synth
    return synth.config4(POOL, n_keys=N_KEYS, seed=0x51554555)


@pytest.fixture(scope="module")
def pool():
    pub, H, S, K, ok = make_pool()
    for a in (pub, H, S, K, ok):
        a.setflags(write=False)
    return pub, H, S, K, ok


def tiled(a, n):
    reps = -(-n // len(a))
    return np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n])


def bits(buf, n):
    return np.unpackbits(buf.to_host(), bitorder="little")[:n].astype(bool)


def context_like_the_benchmark(v, pool, n):
    """bench.py's order: register_keys, to_device x 3, reserve, then the four
    library streams; and one small chunked host-buffer verify, so that the
    context's copy stream and second compute stream exist as well."""
    pub, H, S, K, ok = pool
    assert v.register_keys(pub).all()
    m = n + 3 * SHIFT
    dev = [v.to_device(0, tiled(a, m)) for a in (H, S, K)]
    v.reserve(n)
    streams = [v.stream_create(0) for _ in range(4)]
    os.environ["PBFTV_HOST_CHUNK"] = "2048"  # (read at every call) 4096 signatures = two chunks
    try:
        assert (v.verify_batch(H[:4096], S[:4096], K[:4096]) == ok[:4096]).all()
    finally:
        del os.environ["PBFTV_HOST_CHUNK"]
    return dev, streams, tiled(ok, m)


def enqueue(v, dev, j, n, bitmap, stream):
    dh, ds, dk = dev
    off = SHIFT * j
    v.verify_batch_dev(0, dh.ptr + 32 * off, ds.ptr + 64 * off, dk.ptr + 4 * off, n, bitmap.ptr, stream=stream)


def independence(pool):
    """[(a, b, t_A ms, t_B ms)] for every ordered pair of four library streams,
    after checking every bitmap the timed batches wrote."""
    from simple_pbft_amd import Verifier
    out = []
    with Verifier(device_mask=1) as v:
        dev, streams, want = context_like_the_benchmark(v, pool, N_BIG)
        big = [v.alloc(0, N_BIG // 8 + 1) for _ in streams]
        small = [v.alloc(0, N_SMALL // 8 + 1) for _ in streams]
        for j, st in enumerate(streams):  # each stream's scratch is allocated at its first batch
            enqueue(v, dev, j, N_BIG, big[j], st)
            enqueue(v, dev, j, N_SMALL, small[j], st)
            v.stream_wait(0, st)
        for a in range(4):
            for b in range(4):
                if a == b:
                    continue
                small[b].zero()
                big[a].zero()
                v.sync(0)
                t0 = time.perf_counter()
                for _ in range(DEPTH):
                    enqueue(v, dev, a, N_BIG, big[a], streams[a])
                enqueue(v, dev, b, N_SMALL, small[b], streams[b])
                v.stream_wait(0, streams[b])
                t_b = time.perf_counter() - t0
                v.stream_wait(0, streams[a])
                t_a = time.perf_counter() - t0
                assert (bits(small[b], N_SMALL) == want[SHIFT * b:SHIFT * b + N_SMALL]).all()
                assert (bits(big[a], N_BIG) == want[SHIFT * a:SHIFT * a + N_BIG]).all()
                out.append((a, b, t_a * 1e3, t_b * 1e3))
        for st in streams:
            v.stream_destroy(0, st)
    return out


def interleaved(pool, n, rounds=3):
    """Batches of n round-robin over four library streams, each stream with its
    own inputs and bitmap; every bitmap against the construction."""
    from simple_pbft_amd import Verifier
    with Verifier(device_mask=1) as v:
        dev, streams, want = context_like_the_benchmark(v, pool, n)
        maps = [v.alloc(0, n // 8 + 1) for _ in streams]
        for _ in range(rounds):
            for j, st in enumerate(streams):
                enqueue(v, dev, j, n, maps[j], st)
        for st in streams:
            v.stream_wait(0, st)
        for j in range(4):
            got = bits(maps[j], n)
            exp = want[SHIFT * j:SHIFT * j + n]
            assert (got == exp).all(), f"n={n} stream {j}: {int((got != exp).sum())} bits differ"
            assert not exp.all() and exp.any()
        for st in streams:
            v.stream_destroy(0, st)


def child(mode, pool, tmp_path, *args):
    """This file's __main__ in a fresh process with PBFTV_STREAM_QUEUE=shared."""
    npz = os.path.join(str(tmp_path), "pool.npz")
    np.savez(npz, *pool)
    env = dict(os.environ, PBFTV_STREAM_QUEUE="shared")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, npz, *map(str, args)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def report(kind, rows):
    t_a = [r[2] for r in rows]
    t_b = [r[3] for r in rows]
    ratio = [r[3] / r[2] for r in rows]
    print(f"[{kind}] t_A {min(t_a):.3f}..{max(t_a):.3f} ms, t_B {min(t_b):.3f}..{max(t_b):.3f} ms, "
          f"t_B / t_A {min(ratio):.3f}..{max(ratio):.3f}")
    for a, b, ta, tb in rows:
        print(f"[{kind}]   A = stream {a}, B = stream {b}: t_A {ta:.3f} ms, t_B {tb:.3f} ms, ratio {tb / ta:.3f}")


def test_b_finishes_long_before_a(pool):
    """16 batches of 262,144 on A, then one of 4,096 on B: t_B <= 0.5 t_A for
    every ordered pair.  On one hardware queue B runs after A (t_B >= t_A); on
    its own it needs a few comb-block lifetimes beside A's ~5 ms.

    Measured on an MI355X: t_A 4.46-5.34 ms, t_B 0.36-0.64 ms, ratio
    0.080-0.120 over the twelve pairs."""
    rows = independence(pool)
    report("own queue", rows)
    assert len(rows) == 12
    for a, b, t_a, t_b in rows:
        assert t_b <= 0.5 * t_a, f"A = stream {a}, B = stream {b}: t_B {t_b:.3f} ms, t_A {t_a:.3f} ms"


def test_shared_knob_restores_plain_streams(pool, tmp_path):
    """PBFTV_STREAM_QUEUE=shared: the same run in a fresh process; the results
    are checked there, the ratio is only recorded (plain streams may or may not
    land on one queue, depending on what the process created before).

    Measured on an MI355X: the first and the second stream shared a queue
    (t_B / t_A 0.997 and 0.998, t_B 4.9-5.1 ms); the other ten pairs 0.080-0.092."""
    rows = child("independence", pool, tmp_path)["rows"]
    report("shared", rows)
    assert len(rows) == 12


@pytest.mark.parametrize("n", [s[0] for s in SIZES], ids=[f"{s[0]}" for s in SIZES])
def test_interleaved_batches_are_exact(pool, n):
    interleaved(pool, n)


def test_interleaved_batches_are_exact_shared(pool, tmp_path):
    assert child("interleaved", pool, tmp_path, 32768)["ok"] is True


def test_more_streams_than_dedicated_queues(pool):
    """Ten streams (two past the cap: plain ones), a batch on each, destroyed,
    ten again, a batch on each, exact both times; then pbftv_close."""
    from simple_pbft_amd import Verifier
    pub, H, S, K, ok = pool
    n = N_SMALL
    v = Verifier(device_mask=1)
    try:
        assert v.register_keys(pub).all()
        m = n + 9 * 512
        dev = [v.to_device(0, tiled(a, m)) for a in (H, S, K)]
        dh, ds, dk = dev
        maps = [v.alloc(0, n // 8 + 1) for _ in range(10)]
        for rnd in range(2):
            streams = [v.stream_create(0) for _ in range(10)]
            assert len(set(streams)) == 10
            for b in maps:
                b.zero()
            for j, st in enumerate(streams):
                off = 512 * j
                v.verify_batch_dev(0, dh.ptr + 32 * off, ds.ptr + 64 * off, dk.ptr + 4 * off, n, maps[j].ptr, stream=st)
            for j, st in enumerate(streams):
                v.stream_wait(0, st)
                assert (bits(maps[j], n) == ok[512 * j:512 * j + n]).all(), (rnd, j)
            for st in streams:
                v.stream_destroy(0, st)
    finally:
        v.close()  # (pbftv_close returns nothing; a failure inside it would abort or hang here)
    assert v.handle is None


if __name__ == "__main__":
    mode, npz = sys.argv[1], np.load(sys.argv[2])
    data = tuple(npz[k] for k in npz.files)
    if mode == "independence":
        print(json.dumps({"rows": independence(data)}))
    elif mode == "interleaved":
        interleaved(data, int(sys.argv[3]))
        print(json.dumps({"ok": True}))
    else:
        raise SystemExit(f"unknown mode {mode}")
