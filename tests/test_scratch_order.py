"""The order in which streams use a device's shared scratch
(simple_pbft_amd/csrc/host/scratch_order.h, taken through a ScratchLease at
every scratch user of pbftv_api.cpp), driven on the host by
tests/cpp/test_scratch_order.cpp under AddressSanitizer and UBSan: every
sequence of up to 5 uses over the library's stream and two others, each ended
by a release or by an early exit; a use on another stream than the previous
user's waits for an event recorded on that stream after its work, back-to-back
uses on the library's stream record nothing, and no early exit leaves the
scratch attributed to an older stream."""
from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "test_scratch_order.cpp")
HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "host", "scratch_order.h")
BIN = os.path.join(CPP, "test_scratch_order")
API = os.path.join(ROOT, "simple_pbft_amd", "csrc", "pbftv_api.cpp")


def build_scratch_order_test() -> str:
    if os.path.exists(BIN) and all(os.path.getmtime(s) <= os.path.getmtime(BIN) for s in (SRC, HDR)):
        return BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", BIN, SRC, "-I", os.path.dirname(HDR)], check=True)
    return BIN


def test_every_sequence_of_uses_is_ordered():
    p = subprocess.run([build_scratch_order_test()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert " 0 failed" in p.stdout
    assert int(p.stdout.split("scratch_order: ")[1].split()[0]) > 50000


def test_header_holds_no_hip():
    with open(HDR) as f:
        code = "\n".join(line.split("//")[0] for line in f)
    assert not re.search(r"\bhip[A-Z_]", code)


def test_scratch_users_go_through_the_lease():
    """In pbftv_api.cpp the order's acquire and release, and the event calls
    behind them, are written once: in the lease's operations."""
    with open(API) as f:
        src = f.read()
    assert "scratch_acquire" not in src and "scratch_release" not in src
    assert not re.search(r"scratch\s*\.\s*(acquire|release)\s*\(", src)
    ops = src.split("struct ScratchOps {", 1)[1].split("\n};\n", 1)[0]
    rest = src.replace(ops, "")
    assert "hipEventRecord(ev, st)" in ops and "hipStreamWaitEvent(st, ev, 0)" in ops
    assert "ScratchOps" in rest and "ScratchOps::" not in rest  # named by the lease's type alone
    # the seven users: verify, carried-key verify, DER verify, sign, sign-DER,
    # the SHA-256 length order on a device buffer and in the host digest path
    assert len(re.findall(r"\bScratchLease lease\(", src)) == 7
    assert src.count("lease.acquire()") == 7
    # a stream's own VerifyScratch or the shared one: one lookup
    assert src.count("d.stream_scratch.find(st)") == 1


def test_dev_prologue_is_written_once():
    with open(API) as f:
        src = f.read()
    assert src.count('"bad context or device index"') == 1
    assert "sign_dev_args" not in src
