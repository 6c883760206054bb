#!/usr/bin/env python3
"""What signing on the GPU costs beside verifying there, on one GPU.

The batch: n distinct 32-byte hashes signed under `--keys` private keys (the
keys of tools/synth.py's config 4, so the registered verify of the same run
checks what the signer made).  In one process, device-resident buffers, HIP
events on the context stream, medians of `--steps` steps after `--warmup`:

  a  pbftv_ecdsa_p256_sign_batch_dev: signs per second;
  b  pbftv_ecdsa_p256_verify_batch_dev of those signatures under the matching
     registered keys: verifies per second (the steps alternate: sign, verify,
     sign again), and the ratio of the two;
  c  the sign kernels alone (timing id PBFTV_K_ECDSA_SIGN, per stage: nonce,
     comb, tail), a pass of its own;
  d  the DER form's step (the writer's kernel on top);
  e  the one-core CPU signing rate of the library the CPU verify baseline of
     bench.py --full uses (OpenSSL 3 libcrypto: ECDSA_do_sign on one thread,
     tools/synth_sign.c), over a bounded sample.

Before and after the timed steps every signature is checked: the verify's
accept bits are all ones, a sample of rows equals tests/rfc6979_model.py byte
for byte, and the DER slots parse back to the r||s rows.  Prints one JSON
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rfc6979_model as model  # noqa: E402
import synth  # noqa: E402
from simple_pbft_amd import Verifier  # noqa: E402
from simple_pbft_amd.pbftv import lib  # noqa: E402

SEED = 0x50424654  # synth.config4's


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=20000)
    ap.add_argument("--model-sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    signer = synth.Signer(a.keys, SEED)
    priv, pub = signer.priv.copy(), signer.pub.copy()
    rng = np.random.default_rng(SEED)
    H = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32).copy()
    K = (np.arange(n) % a.keys).astype(np.uint32)
    res = {"metric": "ecdsa_sign", "n": n, "keys": a.keys, "steps": a.steps, "warmup": a.warmup}
    L = lib()

    # (e) one core of OpenSSL signing
    B = synth._batch_signer()
    if B is not None:
        m = min(a.cpu_sample, n)
        out = np.zeros((m, 64), np.uint8)
        t0 = time.perf_counter()
        rc = B.synth_sign_batch(priv.ctypes.data, a.keys, H.ctypes.data, K.ctypes.data, m, out.ctypes.data, 1)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        res["cpu_sign_one_core"] = {"value": m / dt, "unit": "signs/s", "sample": m, "seconds": dt,
                                    "kind": "OpenSSL 3 libcrypto ECDSA_do_sign, 1 thread (tools/synth_sign.c)"}

    hip = ctypes.CDLL("libamdhip64.so")  # the runtime libpbftv.so already loaded (same soname)
    vp = ctypes.c_void_p

    def hip_ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    nb = (n + 7) // 8
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(priv).all()
        assert v.register_keys(pub).all()
        st = vp(v.stream(0))
        dh, dk = v.to_device(0, H), v.to_device(0, K)
        dsig, dok, dbm = v.alloc(0, 64 * n + 64), v.alloc(0, nb + 8), v.alloc(0, nb + 8)
        dder, dlen = v.alloc(0, 72 * n + 64), v.alloc(0, 4 * n + 64)

        def step_sign():
            v.sign_batch_dev(0, dh.ptr, dk.ptr, n, dsig.ptr, dok.ptr)

        def step_verify():
            v.verify_batch_dev(0, dh.ptr, dsig.ptr, dk.ptr, n, dbm.ptr)

        def step_der():
            v.sign_der_batch_dev(0, dh.ptr, dk.ptr, n, dder.ptr, dlen.ptr)

        def bits(buf):
            return np.unpackbits(buf.to_host(nb), bitorder="little")[:n].astype(bool)

        def checked():
            """signatures not ok, not accepted by the verify, sampled rows that differ from the model"""
            dsig.zero()
            dok.zero()
            dbm.zero()
            step_sign()
            step_verify()
            v.sync(0)
            sig = dsig.to_host(64 * n).reshape(n, 64)
            pick = np.linspace(0, n - 1, min(a.model_sample, n)).astype(np.int64)
            wrong = sum(model.sign_bytes(H[i].tobytes(), int.from_bytes(priv[K[i]].tobytes(), "big")) !=
                        sig[i].tobytes() for i in pick)
            return {"not_signed": int((~bits(dok)).sum()), "not_verified": int((~bits(dbm)).sum()),
                    "model_mismatches": int(wrong), "model_sample": int(len(pick))}

        res["check_before"] = checked()

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

        # (a), (b), (d): the steps, alternating
        step = {"sign_batch_dev": timed(step_sign), "verify_batch_dev": timed(step_verify)}
        step["sign_batch_dev_again"] = timed(step_sign)
        step["sign_der_batch_dev"] = timed(step_der)
        res["step_ms"] = step
        sign_ms = min(step["sign_batch_dev"]["median"], step["sign_batch_dev_again"]["median"])
        res["signs_per_s"] = n / (sign_ms * 1e-3)
        res["verifies_per_s"] = n / (step["verify_batch_dev"]["median"] * 1e-3)
        res["sign_over_verify"] = sign_ms / step["verify_batch_dev"]["median"]
        if "cpu_sign_one_core" in res:
            res["gpu_over_one_cpu_core"] = res["signs_per_s"] / res["cpu_sign_one_core"]["value"]

        # (c) the kernels alone, per stage: events around each launch, a pass of its own
        v.set_kernel_timing(True)
        v.reset_kernel_times()
        for _ in range(a.steps):
            step_sign()
        v.sync(0)
        stages = {}
        for name, stage in (("nonce", 1), ("comb", 2), ("tail", 3)):
            ms, cnt = v.sign_kernel_time_ms(0, stage)
            stages[name + "_ms"] = ms / max(cnt, 1)
            stages[name + "_launches"] = int(cnt)
        v.reset_kernel_times()
        step_der()
        v.sync(0)
        ms, cnt = v.sign_kernel_time_ms(0, 4)
        stages["der_writer_ms"] = ms / max(cnt, 1)
        v.set_kernel_timing(False)
        res["kernel_ms"] = stages

        res["check_after"] = checked()
        # the DER slots parse back to the rows just checked
        sig = dsig.to_host(64 * n)
        der, ln = dder.to_host(72 * n), dlen.to_host(4 * n, dtype=np.uint32)
        back = np.zeros(64 * n, np.uint8)
        off = (72 * np.arange(n)).astype(np.uint64)
        parsed = L.pbftv_ecdsa_der_to_rs_batch(der.ctypes.data, off.ctypes.data, ln.ctypes.data, n, back.ctypes.data)
        res["der"] = {"parsed": int(parsed), "rows_differ": int((back.reshape(n, 64) != sig.reshape(n, 64)).any(axis=1).sum()),
                      "min_len": int(ln.min()), "max_len": int(ln.max())}
        for b in (dh, dk, dsig, dok, dbm, dder, dlen):
            b.free()
    signer.close()

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = 0
    for c in (res["check_before"], res["check_after"]):
        bad += c["not_signed"] + c["not_verified"] + c["model_mismatches"]
    bad += (n - res["der"]["parsed"]) + res["der"]["rows_differ"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
