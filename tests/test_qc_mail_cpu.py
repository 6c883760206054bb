"""simple_pbft_amd/csrc/qc_mail.h on the host (tests/cpp/qc_mail_harness.cpp,
built with g++): the latency path's mailbox protocol, the host's writer against
the armed kernels' reader.  Requests are posted into a heap block of exactly
QcMail::bytes(kQcCap) bytes over a complete earlier request, and every slot's
snapshot is built the way its wave loads it (lanes 0-47 its slot lines, lanes
48-63 the header).  Each check returns its number of failures (and says them on
stderr).  The same source runs as a stand-alone program under
-fsanitize=address,undefined."""
from __future__ import annotations

import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "qc_mail_harness.cpp")
_HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "qc_mail.h")
NS = (1, 3, 8, 9, 67, 128)
N_OLD = (128, 3)  # the request before: every slot and helper filled, or fewer slots than any n > 3
CURS = (2, 0x80000000, 0xFFFFFFFE)
SEED = 0x51C0FFEE


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in (_HDR, _SRC))


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libqc_mail_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    lib.h_qc_mail_bytes.argtypes, lib.h_qc_mail_bytes.restype = [], u64
    for f in (lib.h_qc_check_post, lib.h_qc_check_tearing):
        f.argtypes, f.restype = [u32, u32, u32, u64], ctypes.c_int
    lib.h_qc_check_cancel.argtypes, lib.h_qc_check_cancel.restype = [u32, u64], ctypes.c_int
    lib.h_qc_check_relay.argtypes, lib.h_qc_check_relay.restype = [], ctypes.c_int
    return lib


def test_mailbox_size(H):
    """the layout the armed kernels assume (cap = 128): header, 8 slots of 3 lines, 2 x 128 live words, 128 verdict
    bytes, the arrays (100 B per signature), 32 B of stamps per wave and a spare line"""
    assert H.h_qc_mail_bytes() == 64 + 8 * 192 + 2 * 4 * 128 + 128 + 100 * 128 + 32 * 128 + 64


@pytest.mark.parametrize("n", NS)
def test_posted_request_is_read_back(H, n):
    """every slot ready for the posted number and no other; slots < min(n, 8) decode to the posted hash, r, s, key
    and n; slots >= n ready from line 0 alone; helpers 8..n-1 read the posted inputs from the arrays"""
    for cur in CURS:
        for n_old in N_OLD:
            assert H.h_qc_check_post(n, n_old, cur, SEED + n) == 0, (n, n_old, cur)


@pytest.mark.parametrize("n", NS)
def test_torn_requests_are_not_ready(H, n):
    """every subset of a slot's lines new over the old request: ready iff the lines it needs are new; a line with
    one new and one old tag is never new"""
    for cur in CURS:
        for n_old in N_OLD:
            assert H.h_qc_check_tearing(n, n_old, cur, SEED + n) == 0, (n, n_old, cur)


def test_cancel(H):
    """stop == want cancels, a changed halt cancels, neither does not"""
    for cur in CURS:
        assert H.h_qc_check_cancel(cur, SEED) == 0


def test_relay(H):
    """pack and unpack agree; the "wave 0 left" value is recognised, and only it"""
    assert H.h_qc_check_relay() == 0


def test_stand_alone_program_under_sanitizers():
    """The harness with its own main, built with -fsanitize=address,undefined (host code only): the mailbox is a
    heap block of exactly its size, so a read or write past it by the writer or a snapshot aborts the program."""
    exe = os.path.join(_CPP, "qc_mail_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DQC_MAIL_MAIN", "-o", exe, _SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "qc_mail: 0 failures over 74 checks" in p.stdout
