"""The stage case lists of tests/sign_stage_cases.py on the CPU: their
invariants, and every expected signature that is a real one verified by
oracle/p256.py under its key's public half."""
from __future__ import annotations

import numpy as np

import sign_cases as sc
import sign_stage_cases as ssc
from oracle import p256

N = sc.N


def as_int(ws) -> int:
    return int.from_bytes(np.asarray(ws, np.uint32).tobytes(), "little")


def verifies(h: bytes, d: int, row) -> bool:
    r, s = int.from_bytes(bytes(row[:32]), "big"), int.from_bytes(bytes(row[32:]), "big")
    return p256.verify(h, r, s, *p256.pubkey(d))


def test_nonce_rows():
    hashes, kidx, ds, rec, want = ssc.nonce_rows()
    cases = sc.drbg_cases()
    n = len(cases)
    assert n == len(sc.H1_SEAM) * len(sc.D_ENDS) + 64 and cases[:24] == tuple(
        (d, h) for h in sc.H1_SEAM for d in sc.D_ENDS)
    assert kidx.tolist() == list(range(n)) and len(ds) == n  # every d its own key
    first = sc.drbg_expected(cases, 1)[:, 0]
    for i in range(n):
        k, kinv = as_int(want[i, ssc.K:ssc.K + 8]), as_int(want[i, ssc.KINV:ssc.KINV + 8])
        assert k == int.from_bytes(first[i].tobytes(), "big") and 0 < k < N and k * kinv % N == 1
        assert want[i, 16:20].tolist() == [ssc.NONCE_READY, 0, 0, 0]
    # h1 = n is h1 = 0 after bits2octets, h1 = n - 1 is not: the seam is in the list
    by = {c: want[i, :8].tolist() for i, c in enumerate(cases)}
    assert by[(1, N)] == by[(1, 0)] and by[(1, N + 1)] == by[(1, 1)] and by[(1, N - 1)] != by[(1, 0)]
    assert rec.shape == (n + 1, ssc.REC_WORDS) and (rec == ssc.blank_records(n)).all()


def test_chain_expected_are_real_signatures():
    want = ssc.chain_expected()
    for i, (d, h) in enumerate(sc.drbg_cases()):
        assert want[i].any() and verifies(sc.be(h), d, want[i]), i


def test_comb_rows():
    rec, want = ssc.comb_rows()
    ks = sc.chosen_k()
    assert rec.shape == want.shape == (len(ks) + 1, ssc.REC_WORDS)
    digits = set()
    for i, k in enumerate(ks):
        assert as_int(rec[i, :8]) == k and as_int(rec[i, 8:16]) * k % N == 1 and rec[i, ssc.STATE] == ssc.NONCE_READY
        r = as_int(want[i, ssc.R:ssc.R + 8])
        assert 0 < r < N and want[i, ssc.STATE] == ssc.R_READY
        digits |= {(k >> (16 * w)) & 0xFFFF for w in range(16)}
    assert {0, 0x7FFF, 0x8000, 0x8001, 0xFFFF} <= digits and N - 1 in ks
    # a few r against a scalar multiplication made here
    for i in (0, 3, len(ks) // 2, len(ks) - 1):
        assert as_int(want[i, ssc.R:ssc.R + 8]) == p256.scalar_mult(ks[i], p256.G)[0] % N
    # the comb owns the state word and r, nothing else
    own = np.zeros(ssc.REC_WORDS, bool)
    own[ssc.STATE] = True
    own[ssc.R:ssc.R + 8] = True
    assert (rec[:, ~own] == want[:, ~own]).all() and (rec[-1] == want[-1]).all()


def test_tail_chosen_rows_keep_nine_tenths_of_the_cross():
    cross, kept = ssc.tail_cross(), ssc.tail_chosen()
    assert len(cross) == len(ssc.TAIL_R) * len(ssc.TAIL_KINV) * len(sc.E_ENDS) * len(sc.D_PAIR) == 160
    assert {1, N - 1, 1 << 32, 1 << 224} < set(ssc.TAIL_R) and {1, 2, N - 1} < set(ssc.TAIL_KINV)
    assert all(0 < v < N for v in ssc.TAIL_R + ssc.TAIL_KINV)
    assert 10 * len(kept) >= 9 * len(cross)
    dropped = set(cross) - {c[:4] for c in kept}
    assert all(ki * (e + r * d) % N == 0 for e, d, r, ki in dropped) and len(dropped) + len(kept) == len(cross)
    hashes, kidx, ds, rec, want = ssc.tail_chosen_rows()
    assert ds == sc.D_PAIR and len(hashes) == len(kept)
    for i, (e, d, r, ki, s) in enumerate(kept):
        assert s and s == ki * (e + r * d) % N == ki * (e % N + r * d) % N
        assert int.from_bytes(hashes[i].tobytes(), "big") == e and ds[kidx[i]] == d
        assert rec[i, ssc.STATE] == ssc.R_READY and as_int(rec[i, 8:16]) == ki and as_int(rec[i, 20:28]) == r
        assert want[i].tobytes() == sc.be(r) + sc.be(s)
    assert {e for e, *_ in kept} == set(sc.E_ENDS)  # e >= n is still there after the drop
    ssc.check_met_rows(rec, kidx, ds)


def test_tail_batch():
    b = ssc.tail_batch()
    n, ds, rec, kidx = ssc.BATCH, b["ds"], b["rec"], b["kidx"]
    assert n == 257 and rec.shape == (n + 1, ssc.REC_WORDS) and (rec[n] == ssc.blank_records(0)[0]).all()
    assert {0, 1, 31, 32, 62, 63, 64, 255} <= set(b["rerun"]) == set(ssc.RERUN_LANES)
    assert set(ssc.FULL_WAVE) <= set(b["rerun"])                               # a wave where every lane reruns
    assert [i for i in ssc.SINGLE_WAVE if i in b["rerun"]] == [255]           # and one with a single rerun lane
    assert not set(b["rerun"]) & set(b["nosig"])
    pairs = ssc.rerun_pairs()
    assert {(p, how) for p, how in b["rerun"].values()} == {(p, how) for p in range(len(pairs))
                                                             for how in ssc.FORGERIES}
    assert [int.from_bytes(h, "big") for h, _ in pairs[21:]] == list(ssc.RERUN_HASHES) == [0, N, sc.TOP]
    for lane, (p, how) in b["rerun"].items():
        h, d = pairs[p]
        assert b["hashes"][lane].tobytes() == h and ds[kidx[lane]] == d and 0 < d < N  # genuine hash, valid key
        k, kinv, r = ssc.genuine(h, d)
        st, rr, kk = rec[lane, ssc.STATE], as_int(rec[lane, 20:28]), as_int(rec[lane, 8:16])
        if how == "met":
            assert st == ssc.WALK_MET and rr != r and kk != kinv and as_int(rec[lane, :8]) != k
        elif how == "r0":
            assert st == ssc.R_READY and rr == 0 and kk == kinv
        else:
            assert st == ssc.R_READY and rr == r and kk == 0
        assert b["ok"][lane] and b["want"][lane].tobytes() == ssc.signature(h, d)
    ssc.check_met_rows(rec, kidx, ds)
    # rows with no signature: state "none", an index at and past the key count, the invalid key
    nvalid = len(ds) - 1
    assert ds[nvalid] == 0 and all(0 < d < N for d in ds[:nvalid])
    assert set(b["nosig"].values()) >= {"none", "past", "big", "invalid"}
    for lane, how in b["nosig"].items():
        assert not b["ok"][lane] and not b["want"][lane].any()
        assert rec[lane, ssc.STATE] == ssc.NONE or kidx[lane] >= nvalid
        assert rec[lane, ssc.STATE] != ssc.WALK_MET
    assert sorted(set(kidx[list(b["nosig"])].tolist()) - set(range(nvalid))) == [nvalid, nvalid + 1, ssc.BIG]
    # every signed row is a real signature of its hash under its key: verified once per distinct pair
    seen = set()
    for i in range(n):
        if not b["ok"][i]:
            continue
        h, d = b["hashes"][i].tobytes(), ds[kidx[i]]
        assert b["want"][i].tobytes() == ssc.signature(h, d)
        if (h, d) not in seen:
            seen.add((h, d))
            assert verifies(h, d, b["want"][i]), i
    assert len(seen) == ssc.ORDINARY + len(ssc.RERUN_HASHES)
    # ordinary rows carry their genuine record
    for i in (2, 129, 192, 253):
        k, kinv, r = ssc.genuine(b["hashes"][i].tobytes(), ds[kidx[i]])
        assert [as_int(rec[i, a:a + 8]) for a in (0, 8, 20)] == [k, kinv, r] and rec[i, ssc.STATE] == ssc.R_READY
    assert ssc.bitmap(b["ok"]).tolist() == np.packbits(b["ok"], bitorder="little").tolist()


def test_key_block_layout():
    blk = ssc.key_block((1, 0, N - 1, N))
    assert blk[32:].tolist() == [1, 0, 1, 0] and blk[0] == 1 and not blk[1:16].any() and not blk[24:32].any()
    assert as_int(blk[16:24]) == N - 1
