#!/usr/bin/env python3
"""Throughput of the verify under unregistered keys
(pbftv_ecdsa_p256_verify_pubkey_batch_dev, or with --key-format compressed /
uncompressed pbftv_ecdsa_p256_verify_wirekey_batch_dev on the same keys in SEC1
wire form) on one GPU, beside the CPU baseline on the same inputs.

The batch: n OpenSSL-signed signatures (tools/synth.py config 4: all distinct,
1 % corrupted over the eight corruption classes) over a pool of `--keys`
keys, each signature carrying pub[key_idx[i]]; device-resident.  Every accept
bit of the first step is checked against the construction, and a sample
against the oracle.  One step = one _dev call on the context stream; the steps
are timed one by one with HIP events on that stream after warm-up, and the
median is reported.  A second pass with the library's kernel timing on gives
the stage-1 and ladder kernels' own times.  The CPU figure is bench.py's
cpu_baseline: the OpenSSL stand-in (oracle/openssl_standin.c) on host threads.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synth  # noqa: E402
from simple_pbft_amd import KEY_SEC1_COMPRESSED, KEY_SEC1_UNCOMPRESSED, KEY_XY, Verifier  # noqa: E402

K_SCALARS, K_VARBASE = 0, 5
KEY_FORMATS = {"xy": KEY_XY, "compressed": KEY_SEC1_COMPRESSED, "uncompressed": KEY_SEC1_UNCOMPRESSED}


def wire_keys(P, fmt):
    """the X||Y keys P (n, 64) as a packed column in fmt (elliptic.Marshal / MarshalCompressed's bytes)"""
    if fmt == KEY_XY:
        return P
    if fmt == KEY_SEC1_UNCOMPRESSED:
        return np.ascontiguousarray(np.concatenate([np.full((len(P), 1), 4, np.uint8), P], axis=1))
    return np.ascontiguousarray(np.concatenate([(2 + (P[:, 63:64] & 1)).astype(np.uint8), P[:, :32]], axis=1))


def cpu_batch(so_name, fn_name, pub, H, S, K, sample, threads):
    so = os.path.join(ROOT, "oracle", so_name)
    if not os.path.exists(so):
        return None, None
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    fn = getattr(L, fn_name)
    fn.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, ctypes.c_int]
    h, s, k = (np.ascontiguousarray(a[:sample]) for a in (H, S, K))
    bm = np.zeros((sample + 7) // 8, np.uint8)
    t0 = time.perf_counter()
    fn(h.ctypes.data, s.ctypes.data, k.ctypes.data, sample, pub.ctypes.data, len(pub), bm.ctypes.data, threads)
    dt = time.perf_counter() - t0
    return np.unpackbits(bm, bitorder="little")[:sample].astype(bool), dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-sample", type=int, default=262144)
    ap.add_argument("--oracle-sample", type=int, default=8192)
    ap.add_argument("--key-format", choices=sorted(KEY_FORMATS), default="xy",
                    help="how each signature's key is carried (xy: the pubkey entry point)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.steps >= 5 and a.keys >= 1

    pub, H, S, K, ok = synth.config4(a.n, n_keys=a.keys)
    P = np.ascontiguousarray(pub[K])
    n = a.n
    fmt = KEY_FORMATS[a.key_format]
    W = wire_keys(P, fmt)
    res = {"metric": "ecdsa_p256_verify_pubkey_batch" if fmt == KEY_XY else "ecdsa_p256_verify_wirekey_batch",
           "key_format": a.key_format, "key_bytes": int(W.shape[1]), "n": n, "keys": a.keys, "steps": a.steps,
           "warmup": a.warmup, "corrupted": int((~ok).sum())}

    hip = ctypes.CDLL("libamdhip64.so")  # the runtime libpbftv.so already loaded (same soname)
    vp = ctypes.c_void_p

    def hip_ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    with Verifier(device_mask=1) as v:
        st = vp(v.stream(0))
        dh, ds, dp = v.to_device(0, H), v.to_device(0, S), v.to_device(0, W)
        db = v.alloc(0, (n + 7) // 8 + 8)
        db.zero()

        def step():
            if fmt == KEY_XY:
                v.verify_pubkey_batch_dev(0, dh.ptr, ds.ptr, dp.ptr, n, db.ptr)
            else:
                v.verify_wirekey_batch_dev(0, dh.ptr, ds.ptr, dp.ptr, fmt, n, db.ptr)

        step()  # first use: the G table, the scratch
        v.sync(0)
        got = np.unpackbits(db.to_host((n + 7) // 8), bitorder="little")[:n].astype(bool)
        res["mismatches_vs_construction"] = int((got != ok).sum())
        m = min(a.oracle_sample, n)
        ob, _ = cpu_batch("liboracle.so", "oracle_ecdsa_p256_verify_batch", pub, H, S, K, m, a.cpu_threads)
        res["oracle_sample"] = m
        res["mismatches_vs_oracle"] = None if ob is None else int((got[:m] != ob).sum())
        for _ in range(a.warmup):
            step()
        v.sync(0)
        ev = [(vp(), vp()) for _ in range(a.steps)]
        for e0, e1 in ev:
            hip_ok(hip.hipEventCreate(ctypes.byref(e0)))
            hip_ok(hip.hipEventCreate(ctypes.byref(e1)))
        for e0, e1 in ev:
            hip_ok(hip.hipEventRecord(e0, st))
            step()
            hip_ok(hip.hipEventRecord(e1, st))
        v.sync(0)
        ms = []
        for e0, e1 in ev:
            f = ctypes.c_float()
            hip_ok(hip.hipEventElapsedTime(ctypes.byref(f), e0, e1))
            ms.append(float(f.value))
            hip.hipEventDestroy(e0)
            hip.hipEventDestroy(e1)
        again = np.unpackbits(db.to_host((n + 7) // 8), bitorder="little")[:n].astype(bool)
        res["mismatches_after_timed_steps"] = int((again != ok).sum())
        med = statistics.median(ms)
        res.update(ms_per_step=med, ms_min=min(ms), ms_max=max(ms), value=n / (med * 1e-3), unit="verifies/s")
        # the kernels' own times (events around each launch: a pass of its own)
        v.set_kernel_timing(True)
        v.reset_kernel_times()
        for _ in range(5):
            step()
        v.sync(0)
        t_s, c_s = v.kernel_time_ms(0, K_SCALARS)
        t_v, c_v = v.kernel_time_ms(0, K_VARBASE)
        v.set_kernel_timing(False)
        res["kernel_ms"] = {"scalars": t_s / max(c_s, 1), "varbase": t_v / max(c_v, 1)}
        for b in (dh, ds, dp, db):
            b.free()

    sample = min(a.cpu_sample, n) // 512 * 512 or n
    cb, dt = cpu_batch("libopenssl_standin.so", "standin_ecdsa_p256_verify_batch", pub, H, S, K, sample, a.cpu_threads)
    if cb is not None:
        res["cpu_baseline"] = {"kind": "openssl_standin", "value": sample / dt, "unit": "verifies/s",
                               "cores": a.cpu_threads, "sample": sample, "seconds": dt,
                               "mismatches_vs_construction": int((cb != ok[:sample]).sum())}
        res["vs_cpu_baseline"] = res["value"] / res["cpu_baseline"]["value"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = res["mismatches_vs_construction"] or res["mismatches_after_timed_steps"] or res["mismatches_vs_oracle"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
