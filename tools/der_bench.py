#!/usr/bin/env python3
"""What parsing DER signatures on the device is worth, on one GPU.

The batch: n OpenSSL-signed signatures (tools/synth.py config 4: all distinct,
1 % corrupted) over `--keys` registered keys, each DER-encoded as
ecdsa.SignASN1 would (oracle/der.encode) into one blob with offsets and
lengths.  Reported:

  a  host pbftv_ecdsa_der_to_rs_batch over the whole batch (ms, `--passes` passes);
  b  the k_der_to_rs kernel alone (PBFTV_K_ECDSA_DER, ms per launch), beside the
     bytes it moves and the time those bytes take at the HBM rate a float4
     copy reaches on an MI355X (6.29 TB/s);
  c  one verify_der_batch_dev step against one verify_batch_dev step on the
     same inputs (HIP events on the context stream, medians);
  d  host verify_der_batch from pinned memory against the route a caller had
     before: pbftv_ecdsa_der_to_rs_batch, then verify_batch of the r||s (both
     timed end to end, alternating, `--passes` times each).

Every accept bit is checked against the construction before and after the
timed steps, and the device's r||s against the host parse.  Prints one JSON
line; --out also writes it to a file.
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
from oracle import der as oder  # noqa: E402
from simple_pbft_amd import DerColumn, Verifier  # noqa: E402
from simple_pbft_amd.pbftv import lib  # noqa: E402

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X's HBM3E (8.0 TB/s spec)


def der_column(S):
    ders = [oder.encode(int.from_bytes(r[:32].tobytes(), "big"), int.from_bytes(r[32:].tobytes(), "big")) for r in S]
    return DerColumn(ders)


def bits_of(buf, n):
    return np.unpackbits(buf.to_host((n + 7) // 8), bitorder="little")[:n].astype(bool)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    pub, H, S, K, ok = synth.config4(n, n_keys=a.keys)
    col = der_column(S)
    res = {"metric": "ecdsa_der_signatures", "n": n, "keys": a.keys, "steps": a.steps, "warmup": a.warmup,
           "corrupted": int((~ok).sum()), "der_bytes": int(col.blob.nbytes)}
    L = lib()

    def host_parse(out):
        got = L.pbftv_ecdsa_der_to_rs_batch(col.blob.ctypes.data, col.off.ctypes.data, col.len.ctypes.data, n,
                                            out.ctypes.data)
        assert got == n, got

    # (a) the host parse
    rs_host = np.zeros((n, 64), np.uint8)
    t = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        host_parse(rs_host)
        t.append((time.perf_counter() - t0) * 1e3)
    assert (rs_host == S).all()
    res["host_parse_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}

    hip = ctypes.CDLL("libamdhip64.so")  # the runtime libpbftv.so already loaded (same soname)
    vp = ctypes.c_void_p

    def hip_ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    with Verifier(device_mask=1) as v:
        assert v.register_keys(pub).all()
        st = vp(v.stream(0))
        dh, ds, dk = v.to_device(0, H), v.to_device(0, S), v.to_device(0, K)
        dblob, doff, dlen = v.to_device(0, col.blob), v.to_device(0, col.off), v.to_device(0, col.len)
        drs = v.alloc(0, 64 * n)
        db = v.alloc(0, (n + 7) // 8 + 8)
        db.zero()

        def step_rs():
            v.verify_batch_dev(0, dh.ptr, ds.ptr, dk.ptr, n, db.ptr)

        def step_der():
            v.verify_der_batch_dev(0, dh.ptr, dblob.ptr, doff.ptr, dlen.ptr, dk.ptr, n, db.ptr)

        def checked(step):
            db.zero()
            step()
            v.sync(0)
            return int((bits_of(db, n) != ok).sum())

        res["mismatches_before"] = {"rs": checked(step_rs), "der": checked(step_der)}
        v.der_to_rs_batch_dev(0, dblob.ptr, doff.ptr, dlen.ptr, n, drs.ptr)
        v.sync(0)
        res["rs_mismatches_vs_host_parse"] = int((drs.to_host().reshape(n, 64) != rs_host).any(axis=1).sum())

        def timed(step):
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
            return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}

        # (c) the steps, alternating
        res["step_ms"] = {"verify_batch_dev": timed(step_rs), "verify_der_batch_dev": timed(step_der)}
        res["step_ms"]["verify_batch_dev_again"] = timed(step_rs)
        # (b) the kernel alone: events around each launch, a pass of its own
        v.set_kernel_timing(True)
        v.reset_kernel_times()
        for _ in range(a.steps):
            v.der_to_rs_batch_dev(0, dblob.ptr, doff.ptr, dlen.ptr, n, drs.ptr)
        v.sync(0)
        t_k, c_k = v.der_kernel_time_ms(0)
        v.set_kernel_timing(False)
        moved = int(col.blob.nbytes) + 12 * n + 64 * n
        res["kernel"] = {"der_to_rs_ms": t_k / max(c_k, 1), "launches": int(c_k), "bytes_moved": moved,
                         "floor_ms_at_hbm_copy_rate": moved / (HBM_COPY_TBS * 1e12) * 1e3,
                         "hbm_copy_rate_tb_s": HBM_COPY_TBS}
        res["mismatches_after"] = {"rs": checked(step_rs), "der": checked(step_der)}

        # (d) the host forms from pinned memory, alternating
        ph, pk = v.pinned(H), v.pinned(K)
        pblob, poff, plen = v.pinned(col.blob), v.pinned(col.off), v.pinned(col.len)
        prs = v.pinned(np.zeros((n, 64), np.uint8))
        pcol = DerColumn(blob=pblob.a, off=poff.a, length=plen.a)
        bm = np.zeros((n + 7) // 8 + 1, np.uint8)

        def host_der():
            rc = L.pbftv_ecdsa_p256_verify_der_batch(v._h, ph.ptr, *pcol.args(), pk.ptr, n, bm.ctypes.data)
            assert rc == 0, rc

        def host_parse_then_verify():
            got = L.pbftv_ecdsa_der_to_rs_batch(pblob.ptr, poff.ptr, plen.ptr, n, prs.ptr)
            assert got == n
            rc = L.pbftv_ecdsa_p256_verify_batch(v._h, ph.ptr, prs.ptr, pk.ptr, n, bm.ctypes.data)
            assert rc == 0, rc

        host = {"verify_der_batch": [], "parse_then_verify_batch": []}
        wrong = {}
        for fn, name in ((host_der, "verify_der_batch"), (host_parse_then_verify, "parse_then_verify_batch")):
            fn()  # warm: buffers, scratch
            wrong[name] = int((np.unpackbits(bm, bitorder="little")[:n].astype(bool) != ok).sum())
        for _ in range(a.passes):
            for fn, name in ((host_der, "verify_der_batch"), (host_parse_then_verify, "parse_then_verify_batch")):
                bm[:] = 0
                t0 = time.perf_counter()
                fn()
                host[name].append((time.perf_counter() - t0) * 1e3)
                wrong[name] += int((np.unpackbits(bm, bitorder="little")[:n].astype(bool) != ok).sum())
        res["host_ms"] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in host.items()}
        res["host_mismatches"] = wrong
        for p in (ph, pk, pblob, poff, plen, prs):
            p.free()
        for b in (dh, ds, dk, dblob, doff, dlen, drs, db):
            b.free()

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = (sum(res["mismatches_before"].values()) + sum(res["mismatches_after"].values()) +
           res["rs_mismatches_vs_host_parse"] + sum(res["host_mismatches"].values()))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
