"""The pending-free list of pbftv_dev_free (simple_pbft_amd/csrc/host/pending_frees.h,
used by reap_frees and pbftv_close), driven on the host by
tests/cpp/test_pending_frees.cpp under AddressSanitizer and UBSan: every
done / not-done pattern of 0..6 entries, an error at each position, marks
passing one at a time; after every call each entry is still listed with all its
marks or was released once with every mark handed back once."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "test_pending_frees.cpp")
HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "host", "pending_frees.h")
BIN = os.path.join(CPP, "test_pending_frees")


def build_pending_frees_test() -> str:
    if os.path.exists(BIN) and all(os.path.getmtime(s) <= os.path.getmtime(BIN) for s in (SRC, HDR)):
        return BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", BIN, SRC, "-I", os.path.dirname(HDR)], check=True)
    return BIN


def test_pending_free_list_conserves_entries_and_marks():
    p = subprocess.run([build_pending_frees_test()], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert " 0 failed" in p.stdout
    assert int(p.stdout.split("pending_frees: ")[1].split()[0]) > 10000


def test_reap_frees_goes_through_the_template():
    """pbftv_api.cpp keeps no list compaction of its own."""
    with open(os.path.join(ROOT, "simple_pbft_amd", "csrc", "pbftv_api.cpp")) as f:
        src = f.read()
    assert src.count("pbftv::reap_pending(") == 2  # reap_frees and pbftv_close
    assert "pending_frees[k++] = std::move" not in src
