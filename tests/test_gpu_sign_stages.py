"""The library's sign kernels one stage at a time (tests/cpp/sign_stage_probe.hip
-> libsign_stage_probe.so, which compiles p256_sign.hip itself with the
library's flags): k_sign_nonce, k_sign_comb, k_sign_tail and k_sign_der on the
records of tests/sign_stage_cases.py -- chosen hashes, nonces, r and k^-1, and
forged records that send a lane through the tail's rerun (sign_slow) while hash
and key stay genuine.  Every word and byte against tests/rfc6979_model.py and
plain integers."""
from __future__ import annotations

import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import sign_cases as sc
import sign_stage_cases as ssc
from conftest import ROOT
from test_sign_cpu import H, gtab  # noqa: F401  (libsign_harness.so and its G table, rebuilt when stale)

pytestmark = pytest.mark.gpu

HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics"]  # the library's
RS_POISON, OK_POISON = 0xA5, 0xEE


@pytest.fixture(scope="module")
def probe(gtab):  # noqa: F811
    d = os.path.join(ROOT, "tests", "cpp")
    so, src = os.path.join(d, "libsign_stage_probe.so"), os.path.join(d, "sign_stage_probe.hip")
    csrc = os.path.join(ROOT, "simple_pbft_amd", "csrc")
    deps = [src, os.path.join(csrc, "p256_sign.hip")] + glob.glob(os.path.join(csrc, "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # as __graft_entry__.build() and the Makefile
        if not shutil.which(hipcc):
            pytest.fail("tests/cpp/libsign_stage_probe.so is missing or older than its sources and there is no "
                        "hipcc to build it: run __graft_entry__.build()")
        subprocess.run([hipcc] + HIPFLAGS + ["-shared", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.sstp_g_table_bytes.restype = u64
    lib.sstp_record_bytes.restype = u32
    lib.sstp_set_g_table.argtypes = [vp]
    lib.sstp_nonce.argtypes = [vp, vp, vp, u32, u64, vp]
    lib.sstp_comb.argtypes = [u64, vp]
    lib.sstp_tail.argtypes = lib.sstp_chain.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp]
    lib.sstp_der.argtypes = [vp, vp, u64, vp, vp]
    assert lib.sstp_g_table_bytes() == gtab.nbytes and lib.sstp_record_bytes() == 4 * ssc.REC_WORDS
    assert lib.sstp_set_g_table(gtab.ctypes.data) == 0
    yield lib
    lib.sstp_release()


def run_tail(probe, hashes, kidx, ds, rec, n, fn="sstp_tail", okbits=True):
    """the first n rows through the tail (or the whole chain).  Returns (records out with the
    guard, r||s rows with the guard row, raw bitmap bytes with their slack)."""
    hashes, kidx = np.ascontiguousarray(hashes[:n]), np.ascontiguousarray(kidx[:n])
    rec = np.ascontiguousarray(np.concatenate([rec[:n], ssc.blank_records(0)]))
    keys = ssc.key_block(ds)
    rs = np.zeros((n + 1, 64), np.uint8)
    bm = np.zeros((n + 7) // 8 + 8, np.uint8) if okbits else None
    assert getattr(probe, fn)(hashes.ctypes.data, kidx.ctypes.data, keys.ctypes.data, len(ds), n, rec.ctypes.data,
                              rs.ctypes.data, bm.ctypes.data if okbits else None) == 0
    return rec, rs, bm


def check_tail(out, rec_in, want, ok, n):
    """rows, bits, padding bits, the guards, and k and k^-1 wiped in EVERY record"""
    rec, rs, bm = out
    assert (rs[:n] == want[:n]).all(), np.nonzero((rs[:n] != want[:n]).any(axis=1))[0]
    assert (rs[n] == RS_POISON).all()                                 # nothing past row n
    nb = (n + 7) // 8
    bits = np.unpackbits(bm[:nb], bitorder="little")
    assert (bits[:n].astype(bool) == ok[:n]).all(), np.nonzero(bits[:n].astype(bool) != ok[:n])[0]
    assert not bits[n:].any() and (bm[nb:] == OK_POISON).all()        # padding bits zero, nothing past the bitmap
    assert (bm[:nb] == ssc.bitmap(ok[:n])).all()
    assert not rec[:n, :16].any(), np.nonzero(rec[:n, :16].any(axis=1))[0]
    assert (rec[:n, 16:] == rec_in[:n, 16:]).all() and (rec[n] == ssc.blank_records(0)[0]).all()


def test_nonce_stage_on_the_seam_hashes_and_end_keys(probe):
    """k_sign_nonce over H1_SEAM x D_ENDS and 64 random pairs: k the model's first
    candidate, k^-1 its inverse mod n, state "nonce ready", candidate 0 -- and the
    words the stage does not own, and the record past the last, unchanged."""
    hashes, kidx, ds, rec_in, want = ssc.nonce_rows()
    n = len(kidx)
    rec, keys = rec_in.copy(), ssc.key_block(ds)
    assert probe.sstp_nonce(hashes.ctypes.data, kidx.ctypes.data, keys.ctypes.data, len(ds), n, rec.ctypes.data) == 0
    assert (rec[:n, :20] == want).all(), np.nonzero((rec[:n, :20] != want).any(axis=1))[0]
    assert (rec[:n, 20:] == rec_in[:n, 20:]).all() and (rec[n] == rec_in[n]).all()


def test_nonce_stage_rows_without_a_key(probe):
    """an index at and past the key count and an invalid key: k and k^-1 zero, state "none" """
    hashes, _, ds, rec_in, want = ssc.nonce_rows()
    n, ds = 70, tuple(ds[:8]) + (0, sc.N)
    kidx = (np.arange(n) % 8).astype(np.uint32)
    bad = {0: 8, 1: 9, 63: 10, 64: ssc.BIG, 69: 11}
    for i, j in bad.items():
        kidx[i] = j
    rec, keys = rec_in[:n + 1].copy(), ssc.key_block(ds)
    assert probe.sstp_nonce(hashes.ctypes.data, kidx.ctypes.data, keys.ctypes.data, len(ds), n, rec.ctypes.data) == 0
    for i in range(n):
        if i in bad:
            assert not rec[i, :16].any() and rec[i, ssc.STATE] == ssc.NONE and not rec[i, 18:20].any(), i
        elif i < 8:
            assert (rec[i, :20] == want[i]).all(), i  # (row i < 8 still has hash i and key i)
        else:
            assert rec[i, ssc.STATE] == ssc.NONCE_READY and rec[i, :16].any(), i
    assert (rec[:n, 20:] == rec_in[:n, 20:]).all() and (rec[n] == rec_in[n]).all()


def test_comb_stage_on_the_chosen_nonces(probe):
    """k_sign_comb over sign_cases.chosen_k(): r = x(kG) mod n and state "r ready";
    k, k^-1 and every other word it does not own unchanged."""
    rec_in, want = ssc.comb_rows()
    rec = rec_in.copy()
    assert probe.sstp_comb(len(rec) - 1, rec.ctypes.data) == 0
    assert (rec == want).all(), np.nonzero((rec != want).any(axis=1))[0]


def test_comb_stage_leaves_other_states_alone(probe):
    rec_in, want = ssc.comb_rows()
    rec_in, want = rec_in[:71].copy(), want[:71].copy()
    rec_in[70] = want[70] = ssc.blank_records(0)[0]  # the guard after 70 rows
    for i, st in ((0, ssc.NONE), (5, ssc.R_READY), (63, ssc.WALK_MET), (64, ssc.NONE), (69, 7)):
        rec_in[i, ssc.STATE] = st
        want[i] = rec_in[i]
    rec = rec_in.copy()
    assert probe.sstp_comb(70, rec.ctypes.data) == 0
    assert (rec == want).all(), np.nonzero((rec != want).any(axis=1))[0]


def test_tail_stage_on_chosen_records(probe):
    """k_sign_tail over chosen (r, k^-1) x E_ENDS x D_PAIR: s = k^-1 (e + r d) mod n
    with e >= n among the hashes and d at both ends, the row r || s, the bit 1."""
    hashes, kidx, ds, rec_in, want = ssc.tail_chosen_rows()
    n = len(kidx)
    assert n >= 144
    check_tail(run_tail(probe, hashes, kidx, ds, rec_in, n), rec_in, want, np.ones(n, bool), n)


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_tail_stage_reruns_and_unsigned_rows(probe, n):
    """Forged records -- "walk met" with junk, r = 0, k^-1 = 0 -- under genuine
    hashes and keys take sign_slow and give the model's RFC 6979 signature, in a
    wave where every lane reruns, in one where a single lane does, and beside
    ordinary and unsigned rows; k and k^-1 are zero in every record afterwards."""
    b = ssc.tail_batch()
    assert n >= 257 or any(i < n for i in b["rerun"])
    check_tail(run_tail(probe, b["hashes"], b["kidx"], b["ds"], b["rec"], n), b["rec"], b["want"], b["ok"], n)


def test_tail_stage_without_a_bitmap(probe):
    b = ssc.tail_batch()
    n = 65
    rec, rs, _ = run_tail(probe, b["hashes"], b["kidx"], b["ds"], b["rec"], n, okbits=False)
    assert (rs[:n] == b["want"][:n]).all() and (rs[n] == RS_POISON).all() and not rec[:n, :16].any()


def test_probe_refuses_a_walk_met_record_without_a_key(probe):
    """the pairing the comb cannot produce never reaches the kernel"""
    b = ssc.tail_batch()
    kidx = b["kidx"][:64].copy()
    lane = next(i for i, (_, how) in sorted(b["rerun"].items()) if how == "met")
    for idx in (len(b["ds"]) - 1, len(b["ds"]), ssc.BIG):
        kidx[lane] = idx
        rec = b["rec"][:65].copy()
        keys, rs, bm = ssc.key_block(b["ds"]), np.zeros((65, 64), np.uint8), np.zeros(16, np.uint8)
        assert probe.sstp_tail(b["hashes"].ctypes.data, kidx.ctypes.data, keys.ctypes.data, len(b["ds"]), 64,
                               rec.ctypes.data, rs.ctypes.data, bm.ctypes.data) == -1


def test_three_stages_chained_on_the_seam_hashes_and_end_keys(probe):
    """nonce, comb and tail in order, as the library launches them, over H1_SEAM x
    D_ENDS and the random pairs: the model's signatures, every bit 1, records wiped."""
    hashes, kidx, ds, rec_in, _ = ssc.nonce_rows()
    n = len(kidx)
    want = ssc.chain_expected()
    rec, rs, bm = run_tail(probe, hashes, kidx, ds, rec_in, n, fn="sstp_chain")
    assert (rs[:n] == want).all(), np.nonzero((rs[:n] != want).any(axis=1))[0]
    assert (rs[n] == RS_POISON).all()
    nb = (n + 7) // 8
    assert (bm[:nb] == ssc.bitmap(np.ones(n, bool))).all() and (bm[nb:] == OK_POISON).all()
    assert not rec[:n, :16].any() and (rec[:n, ssc.STATE] == ssc.R_READY).all() and not rec[:n, ssc.CAND:20].any()
    assert (rec[n] == rec_in[n]).all()


def test_der_writer_over_the_tails_rerun_rows(probe):
    """launch_sign_der over what the tail wrote for the 257-row batch: the reruns'
    rows encode as the model's signatures do, unsigned rows are zero slots of length 0."""
    b = ssc.tail_batch()
    n = ssc.BATCH
    _, rs, bm = run_tail(probe, b["hashes"], b["kidx"], b["ds"], b["rec"], n)
    der = np.zeros((n + 1, 72), np.uint8)
    ln = np.zeros(n + 4, np.uint32)
    assert probe.sstp_der(rs.ctypes.data, bm.ctypes.data, n, der.ctypes.data, ln.ctypes.data) == 0
    for i in range(n):
        enc = sc.der_expected(b["want"][i]) if b["ok"][i] else b""
        assert ln[i] == len(enc) and der[i, :len(enc)].tobytes() == enc and not der[i, len(enc):].any(), i
    assert (der[n] == RS_POISON).all() and (ln[n:] == 0xA5A5A5A5).all()
