#!/usr/bin/env python3
"""Per-step kernel timeline from a rocprofv3 --kernel-trace database: the
dispatches of the last few steps in start order, with each kernel's duration
and the idle gap before it (microseconds).  With --overlap instead: the
hardware queue each stream's kernels ran on, and whether each k_ecdsa_scalars
started while another stream's k_ecdsa_comb was still running
(profiles/r07_overlap_before.txt / _after.txt).

    python tools/rocpd_timeline.py gpurun_out/prof/run_results.db [--last 12] [--skip 0]"""
import argparse
import re
import sqlite3


def short(name):
    m = re.search(r"(k_\w+|__amd_rocclr_\w+)(<[^>]*>)?", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:40]


def overlap(c, last):
    rows = [(short(nm), s, e, st, q) for nm, s, e, st, q in
            c.execute("select name, start, end, stream_id, queue_id from kernels order by start")]
    place = {}
    for nm, s, e, st, q in rows:
        k = place.setdefault((st, q), {})
        k[nm] = k.get(nm, 0) + 1
    print("stream_id queue_id  dispatches by kernel")
    for (st, q), k in sorted(place.items(), key=str):
        print(f"{st!s:>9} {q!s:>8}  " + ", ".join(f"{n} x{v}" for n, v in sorted(k.items())))
    combs = [r for r in rows if r[0].startswith("k_ecdsa_comb")]
    scal = [r for r in rows if r[0].startswith("k_ecdsa_scalars")]
    inside = []
    for nm, s, e, st, q in scal:
        # the comb of ANOTHER stream that was running when this scalar stage started
        hit = [cb for cb in combs if cb[3] != st and cb[1] <= s < cb[2]]
        inside.append((s, e, st, q, hit[0] if hit else None))
    n_in = sum(1 for r in inside if r[4])
    print(f"k_ecdsa_scalars dispatches: {len(scal)}; started inside another stream's k_ecdsa_comb: {n_in}")
    print(f"last {last} k_ecdsa_scalars (times in us from the first of them):")
    t0 = inside[-last][0] if len(inside) >= last else (inside[0][0] if inside else 0)
    for s, e, st, q, cb in inside[-last:]:
        line = f"  scalars stream {st} queue {q}  start {(s - t0) / 1e3:10.2f}  end {(e - t0) / 1e3:10.2f}"
        if cb:
            line += (f"  | inside comb stream {cb[3]} queue {cb[4]}  start {(cb[1] - t0) / 1e3:10.2f}"
                     f"  end {(cb[2] - t0) / 1e3:10.2f}  shared {(min(e, cb[2]) - s) / 1e3:7.2f} us")
        else:
            prev = [cb2 for cb2 in combs if cb2[3] != st and cb2[2] <= s]
            if prev:
                line += f"  | after comb stream {prev[-1][3]} queue {prev[-1][4]} ended, gap {(s - prev[-1][2]) / 1e3:7.2f} us"
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--last", type=int, default=12)
    ap.add_argument("--skip", type=int, default=0, help="drop this many of the newest dispatches first")
    ap.add_argument("--overlap", action="store_true",
                    help="instead: which queue each stream's kernels ran on, and how many k_ecdsa_scalars "
                         "started while another stream's k_ecdsa_comb was still running")
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    if a.overlap:
        return overlap(c, a.last)
    rows = list(c.execute("select name, start, end, vgpr_count, accum_vgpr_count, sgpr_count, lds_size "
                          "from kernels order by start"))
    rows = rows[:len(rows) - a.skip][-a.last:]
    prev = None
    for name, s, e, v, av, sg, lds in rows:
        gap = (s - prev) / 1e3 if prev is not None else 0.0
        print(f"{short(name):40s} dur {(e - s) / 1e3:9.2f} us  gap {gap:7.2f} us  vgpr {v} agpr {av} sgpr {sg} lds {lds}")
        prev = e


if __name__ == "__main__":
    main()
