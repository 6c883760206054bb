"""ConsensusTable::FlushPreparesTally / FlushCommitsTally of the C++ host
mirror (simple_pbft_amd/csrc/host/pbft.h), driven by
tests/cpp/test_tally_mirror.cpp: on random multi-sequence snapshots they give
the same accepted, applied, errors, commits, replies, stages and stored votes
as the existing FlushPrepares / FlushCommits, flush after flush.

The crypto backend is the oracle behind pbft::Crypto (a test double); the
reduce of csrc/tally.h runs on the host."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "test_tally_mirror")
LIB = os.path.join(ROOT, "simple_pbft_amd", "libpbftv.so")
ORACLE = os.path.join(ROOT, "oracle", "liboracle.so")


def build_tally_mirror_test() -> str:
    src = os.path.join(CPP, "test_tally_mirror.cpp")
    host = os.path.join(ROOT, "simple_pbft_amd", "csrc", "host")
    deps = [src, os.path.join(host, "pbft.h"), os.path.join(ROOT, "simple_pbft_amd", "csrc", "tally.h"), LIB, ORACLE]
    for so, d in ((LIB, "simple_pbft_amd"), (ORACLE, "oracle")):
        if not os.path.exists(so):
            subprocess.run(["make", "-C", os.path.join(ROOT, d), "-s", "-j8"], check=True)
    if os.path.exists(BIN) and all(os.path.getmtime(s) <= os.path.getmtime(BIN) for s in deps):
        return BIN
    subprocess.run(
        ["g++", "-O1", "-std=c++17", "-Wall", "-o", BIN, src, "-I", host, "-I", os.path.join(ROOT, "include"),
         "-L", os.path.dirname(LIB), "-lpbftv", "-L", os.path.dirname(ORACLE), "-loracle",
         "-Wl,-rpath,$ORIGIN/../../simple_pbft_amd", "-Wl,-rpath,$ORIGIN/../../oracle", "-lpthread"],
        check=True)
    return BIN


def _run(mode: str, timeout: int) -> str:
    p = subprocess.run([build_tally_mirror_test(), mode], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout
    return p.stdout


def test_tally_flushes_match_the_existing_ones_cpu_double():
    out = _run("oracle", 120)
    assert "oracle: " in out
    # the snapshots do reach quorums, and do hold accepted votes past them (MSGENOUGH)
    assert any(" 0 accepted after the quorum" not in line for line in out.splitlines() if line.startswith("seed "))

