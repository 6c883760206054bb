"""The kernel timing table (simple_pbft_amd/csrc/host/kernel_timers.h: one table
of 11 slots per device behind pbftv_kernel_time_ms, pbftv_der_kernel_time_ms,
pbftv_sign_kernel_time_ms, pbftv_reset_kernel_times and pbftv_close), driven on
the host by tests/cpp/test_kernel_timers.cpp under AddressSanitizer and UBSan
with counting fake events: timing off, launches in several slots, collect,
reset, drop at close, a create failing at the first and at the second event, a
launch that returns an error, a synchronise or elapsed failing at each pair of
a list; after every step each event created was destroyed exactly once or is
still pending, and sums and counts are the script's own."""
from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "test_kernel_timers.cpp")
HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "host", "kernel_timers.h")
BIN = os.path.join(CPP, "test_kernel_timers")
API = os.path.join(ROOT, "simple_pbft_amd", "csrc", "pbftv_api.cpp")


def build_kernel_timers_test() -> str:
    if os.path.exists(BIN) and all(os.path.getmtime(s) <= os.path.getmtime(BIN) for s in (SRC, HDR)):
        return BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", BIN, SRC, "-I", os.path.dirname(HDR)], check=True)
    return BIN


def test_timing_table_conserves_events_and_sums():
    p = subprocess.run([build_kernel_timers_test()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert " 0 failed" in p.stdout
    assert int(p.stdout.split("kernel_timers: ")[1].split()[0]) > 1000


def test_header_holds_no_hip():
    with open(HDR) as f:
        code = "\n".join(line.split("//")[0] for line in f)
    assert not re.search(r"\bhip[A-Z_]|std::function", code)


def test_timing_goes_through_the_one_table():
    """pbftv_api.cpp keeps one statement of the event pair and of its reading:
    no second copy beside Device::timers, and nothing type-erased on the launch path."""
    with open(API) as f:
        src = f.read()
    assert src.count("hipEventElapsedTime") == 1
    assert src.count("hipEventCreate(") == 1  # (the scratch, reader and free marks use hipEventCreateWithFlags)
    assert src.count(".timers.timed(") == 1 and src.count(".timers.collect(") == 1
    assert src.count("->timers.drop(") == 1  # pbftv_close
    launch_wrapper = src.split("hipError_t timed(Device& d", 1)[1].split("\n}\n", 1)[0]
    assert "std::function" not in launch_wrapper
    assert "sign_timed" not in src and "der_collect_times" not in src and "sign_collect_times" not in src
    assert "KernelTimers<hipEvent_t, PBFTV_K_ECDSA_SIGN + kSignStages, TimerOps>" in src  # 7 + 4 slots
