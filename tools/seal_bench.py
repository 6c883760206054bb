#!/usr/bin/env python3
"""Sealing votes in one call against what a caller did before, on one GPU.

The batch: n votes with a 64-hex digest and a short node id (the reference's
shapes), signed under `--keys` signing keys, DER signatures.  In one process,
alternating, `--repeats` times each, wall-clock around the calls:

  baseline  pbftv_digest_vote_batch, then pbftv_ecdsa_p256_sign_der_batch, then
            a C loop on one core that builds every signed wire form with
            pbftv_gojson_vote_signed (tools/seal_baseline.c) -- all three over
            preallocated buffers, each part timed;
  seal      pbftv_seal_votes (PBFTV_SIG_DER) into a pinned buffer sized by the
            header's bound.

Every byte, offset and length of the last repeat's sealed batch is compared
with the baseline's.  Prints one JSON line (medians and ranges in ms); --out
also writes it to a file.  --only seal|baseline runs one side alone (for a
kernel trace of that side).
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simple_pbft_amd import SIG_DER, Verifier  # noqa: E402
from simple_pbft_amd.pbftv import PBFTV_OK, PinnedArray, VoteColumns, lib  # noqa: E402

N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
NODES = (b"Apple", b"MS", b"Google", b"IBM")


def votes_columns(n: int) -> VoteColumns:
    """n votes built column-wise (no per-vote Python objects)."""
    rng = np.random.default_rng(0x5EA1)
    hexd = np.frombuffer(rng.bytes(32 * n).hex().encode(), np.uint8)
    cols = VoteColumns([])
    cols.n = n
    cols.view = np.zeros(n, np.int64)
    cols.seq = np.arange(n, dtype=np.int64) // 4
    cols.type = (1 + np.arange(n) % 2).astype(np.int64)
    cols.digest = (np.ascontiguousarray(hexd), (64 * np.arange(n)).astype(np.uint64), np.full(n, 64, np.uint32))
    nodes = np.frombuffer(b"".join(NODES), np.uint8)
    starts = np.cumsum([0] + [len(x) for x in NODES[:-1]])
    cols.node = (np.ascontiguousarray(nodes), starts[np.arange(n) % 4].astype(np.uint64),
                 np.array([len(x) for x in NODES], np.uint32)[np.arange(n) % 4])
    return cols


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["seal", "baseline"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = lib()
    B = ctypes.CDLL(os.path.join(ROOT, "tools", "libseal_baseline.so"))
    B.seal_baseline_votes.restype = ctypes.c_uint64
    B.seal_baseline_votes.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 12 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    encode = ctypes.cast(L.pbftv_gojson_vote_signed, ctypes.c_void_p)
    priv = np.frombuffer(b"".join((int.from_bytes(hashlib.sha256(b"seal bench key %d" % j).digest(), "big")
                                   % (N_ORDER - 1) + 1).to_bytes(32, "big") for j in range(a.keys)),
                         np.uint8).reshape(a.keys, 32)
    res = {"metric": "seal_votes", "keys": a.keys, "repeats": a.repeats, "sig_format": "der", "sizes": {}}
    bad = 0
    with Verifier(device_mask=1) as v:
        assert v.register_signing_keys(priv).all()
        for n in [int(x) for x in a.sizes.split(",")]:
            cols = votes_columns(n)
            kidx = (np.arange(n) % a.keys).astype(np.uint32)
            cap = n * (120 + 6 * (64 + 6) + 111)  # include/pbftv.h's bound for these columns
            # baseline buffers
            dg = np.zeros((n, 32), np.uint8)
            der, dl = np.zeros((n, 72), np.uint8), np.zeros(n, np.uint32)
            b_out, b_off, b_len = np.zeros(cap, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
            # seal buffers
            pin = PinnedArray(v, (cap,), np.uint8)
            s_off, s_len, s_dg = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 32), np.uint8)
            s_bm = np.zeros((n + 7) // 8, np.uint8)
            s_total = ctypes.c_uint64(0)
            args = cols.args()

            def baseline():
                t0 = time.perf_counter()
                rc = L.pbftv_digest_vote_batch(v._h, n, *args, dg.ctypes.data)
                t1 = time.perf_counter()
                rc |= L.pbftv_ecdsa_p256_sign_der_batch(v._h, dg.ctypes.data, kidx.ctypes.data, n, der.ctypes.data,
                                                        dl.ctypes.data)
                t2 = time.perf_counter()
                total = B.seal_baseline_votes(encode, n, *args, der.ctypes.data, dl.ctypes.data, b_out.ctypes.data,
                                              cap, b_off.ctypes.data, b_len.ctypes.data)
                t3 = time.perf_counter()
                assert rc == PBFTV_OK and total <= cap
                return total, [1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0)]

            def seal():
                t0 = time.perf_counter()
                rc = L.pbftv_seal_votes(v._h, n, *args, kidx.ctypes.data, SIG_DER, pin.ptr, cap, s_off.ctypes.data,
                                        s_len.ctypes.data, ctypes.byref(s_total), s_dg.ctypes.data, s_bm.ctypes.data)
                t1 = time.perf_counter()
                assert rc == PBFTV_OK, rc
                return s_total.value, 1e3 * (t1 - t0)

            if a.only != "seal":
                baseline()  # warm-up: buffers grown, tables built
            if a.only != "baseline":
                seal()
            bt, st = [], []
            b_total = s_tot = None
            for _ in range(a.repeats):
                if a.only != "seal":
                    b_total, t = baseline()
                    bt.append(t)
                if a.only != "baseline":
                    s_tot, t = seal()
                    st.append(t)
            r = {"wire_bytes": int(s_tot if s_tot is not None else b_total)}
            if bt:
                parts = list(zip(*bt))
                r["baseline_ms"] = stats(parts[3])
                r["baseline_parts_ms"] = {"digest_vote_batch": stats(parts[0]), "sign_der_batch": stats(parts[1]),
                                          "gojson_vote_signed_loop_one_core": stats(parts[2])}
            if st:
                r["seal_ms"] = stats(st)
                r["sealed_per_s"] = n / (r["seal_ms"]["median"] * 1e-3)
            if bt and st:
                same = (b_total == s_tot and np.array_equal(b_off, s_off) and np.array_equal(b_len, s_len) and
                        np.array_equal(b_out[:b_total], pin.a[:s_tot]) and np.array_equal(dg, s_dg) and
                        bool(np.unpackbits(s_bm, bitorder="little")[:n].all()))
                r["bytes_equal_baseline"] = bool(same)
                r["seal_over_baseline"] = r["seal_ms"]["median"] / r["baseline_ms"]["median"]
                bad += not same
            res["sizes"][str(n)] = r
            pin.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
