"""simple_pbft_amd/csrc/tally.h on the host (tests/cpp/tally_harness.cpp, built
with g++) against the pure-Python model tests/tally_model.py over every case of
tests/tally_cases.py: every word of the signer sets, every count and every
quorum_at -- with and without the message bitmap, with and without priors.  The
same harness runs as a stand-alone program under -fsanitize=address,undefined
with every row and signer block in a heap block of exactly its size."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import tally_cases as tc
import tally_model as tm
from conftest import ROOT

_CPP = os.path.join(ROOT, "tests", "cpp")
_SRC = os.path.join(_CPP, "tally_harness.cpp")
_HDR = os.path.join(ROOT, "simple_pbft_amd", "csrc", "tally.h")


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in (_HDR, _SRC))


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_CPP, "libtally_harness.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, _SRC], check=True)
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.h_tally.argtypes = [vp, vp, vp, vp, ctypes.c_uint64, u32, u32, u32, vp, vp, vp]
    lib.h_tally.restype = None
    for f in (lib.h_tally_words, lib.h_tally_index_bits):
        f.argtypes, f.restype = [u32], u32
    lib.h_tally_word_mask.argtypes, lib.h_tally_word_mask.restype = [u32, u32], u32
    return lib


def run(H, c, with_msg=True, with_priors=True, with_at=True):
    sig, msg = c.sig_bitmap(), c.msg_bitmap()
    signers = c.priors.copy() if with_priors else None
    count = np.full(c.n_states, 0xEEEEEEEE, np.uint32)
    q_at = np.full(c.n_states, 0xEEEEEEEE, np.uint32)
    H.h_tally(sig.ctypes.data, msg.ctypes.data if with_msg else None, c.key_idx.ctypes.data, c.state_idx.ctypes.data,
              c.n, c.n_states, c.n_signers, c.quorum, signers.ctypes.data if with_priors else None, count.ctypes.data,
              q_at.ctypes.data if with_at else None)
    return signers, count, q_at


def test_model_small_examples():
    """the model itself on cases worked by hand"""
    # 3 signers, quorum 2: votes from signers 2, 2 (duplicate), 0 -> quorum completed by vote 2
    s, c, q = tm.tally([1, 1, 1], None, [2, 2, 0], [0, 0, 0], 2, 3, 2)
    assert s.tolist() == [[0b101], [0]] and c.tolist() == [2, 0] and q.tolist() == [2, tm.NONE]
    # the first copy rejected: the later one is the signer's first
    s, c, q = tm.tally([0, 1, 1], [1, 1, 1], [2, 2, 0], [0, 0, 0], 1, 3, 1)
    assert q.tolist() == [1]
    # priors {0} (and garbage bit 3): signer 0's vote is not fresh; quorum 2 needs one more
    s, c, q = tm.tally([1, 1], None, [0, 1], [0, 0], 1, 3, 2, priors=np.array([[0b1001]], np.uint32))
    assert s.tolist() == [[0b011]] and c.tolist() == [2] and q.tolist() == [1]
    # priors at the quorum, and quorum 0
    assert tm.tally([1], None, [1], [0], 1, 3, 1, priors=np.array([[0b100]], np.uint32))[2].tolist() == [tm.BEFORE]
    assert tm.tally([], None, [], [], 2, 3, 0)[2].tolist() == [tm.BEFORE, tm.BEFORE]
    assert tm.applied([1, 1, 1], None, [2, 2, 0], [0, 0, 0], 2, 3, [1, tm.NONE]) == [True, True, False]


def test_helpers(H):
    for k in list(range(0, 130)) + [1000, 2049, (1 << 28)]:
        assert H.h_tally_words(k) == tm.words(k)
        for w in range(0, tm.words(k) + 2):
            want = sum(1 << b for b in range(32) if 32 * w + b < k)
            assert H.h_tally_word_mask(w, k) == want
    for n in [0, 1, 2, 3, 4, 5, 255, 256, 257, 1 << 20, (1 << 31) + 1, 0xFFFFFFFD]:
        assert H.h_tally_index_bits(n) == (0 if n <= 1 else (n - 1).bit_length())


@pytest.mark.parametrize("n_signers", tc.N_SIGNERS)
def test_header_matches_model(H, n_signers):
    for c in tc.suite(n_signers):
        for with_msg, with_priors in ((True, True), (False, True), (True, False)):
            want = c.expect(with_msg, with_priors)
            signers, count, q_at = run(H, c, with_msg, with_priors)
            if with_priors:
                assert (signers == want[0]).all(), c.name
            assert (count == want[1]).all(), c.name
            assert (q_at == want[2]).all(), (c.name, q_at, want[2])
        # quorum_at not asked for: the rest unchanged
        signers, count, q_at = run(H, c, with_at=False)
        want = c.expect()
        assert (signers == want[0]).all() and (count == want[1]).all() and (q_at == 0xEEEEEEEE).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The harness with its own main, built with -fsanitize=address,undefined
    (host code only): each state's row and signer words in heap blocks of
    exactly their sizes, so a read or write past either aborts the program."""
    exe = os.path.join(_CPP, "tally_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DTALLY_MAIN", "-o", exe, _SRC], check=True)
    path = tmp_path / "corpus.bin"
    cases = states = 0
    with open(path, "wb") as f:
        for c in tc.all_cases():
            if c.n > 300 and c.n_signers not in (33, 2049):
                continue  # the large snapshots of two sizes are enough under the sanitizers
            for with_msg, with_priors in ((True, True), (False, False)):
                want = c.expect(with_msg, with_priors)
                f.write(struct.pack("<6I", c.n, c.n_states, c.n_signers, c.quorum, int(with_msg), int(with_priors)))
                f.write(c.sig_bitmap().tobytes())
                if with_msg:
                    f.write(c.msg_bitmap().tobytes())
                f.write(c.key_idx.tobytes() + c.state_idx.tobytes())
                for s in range(c.n_states):
                    if with_priors:
                        f.write(c.priors[s].tobytes())
                    f.write(want[0][s].tobytes() + struct.pack("<II", int(want[1][s]), int(want[2][s])))
                cases += 1
                states += c.n_states
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "tally: 0 mismatches over %d states of %d cases" % (states, cases) in p.stdout
