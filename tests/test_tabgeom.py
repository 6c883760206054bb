"""tests/tabgeom.py on the CPU: the restated build geometry against the
figures DESIGN.md §3.6 states and against an exact cover of a table's entries,
the rule for which probes may be missing, and -- on the CPU harness's tables
(codes 8 and 11) -- that a probe signature really reads the entry it names:
one flipped bit in that entry turns its accept into a reject."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import tabgeom as tg
from conftest import signed_digits
from test_algo_cpu import H  # noqa: F401  (the CPU harness fixture)

# DESIGN.md §3.6 / p256_algo.h CombGeom: windows per code
K_WIN = {8: 33, 12: 22, 16: 17, 20: 13, 21: 12, 22: 12, 24: 11, 26: 10, 29: 9}


def test_lanes_cover_every_entry_once():
    """Phase-3 lanes of a 2-base build write each entry of each base exactly once."""
    for code in (8, 12, 11):
        g = tg.tabgeom(code)
        nent = g.words // 16
        seen = np.zeros((2, nent), np.int32)
        written = 0
        for lane in range(2 * g.per_base):
            le = tg.lane_entries(code, lane)
            if le is None:
                continue
            (b, win, hi, part), ms = le
            assert len(ms) == g.PC and ms[0] == hi * g.CL + part * g.PC + 1 and ms[-1] <= g.ent(win)
            seen[b, g.base(win) + ms[0] - 1:g.base(win) + ms[-1]] += 1
            written += 1
        assert (seen == 1).all(), code
        assert written * g.PC == 2 * nent
    # narrow top windows leave lanes without entries only in the mixed code
    assert all(tg.lane_entries(8, l) is not None for l in range(tg.tabgeom(8).per_base))
    assert any(tg.lane_entries(11, l) is None for l in range(tg.tabgeom(11).per_base))


def test_geometry_figures():
    """Window counts, table sizes and launch counts as DESIGN.md §3.6 / §3.7 and
    p256_kernels.hip state them."""
    assert set(K_WIN) == set(tg.TABLE_WIDTHS)
    for code, nwin in K_WIN.items():
        g = tg.tabgeom(code)
        assert g.kWin == nwin and sum(g.widths) >= 257
        assert g.CL * g.NH == g.kEnt and g.SL * g.SEG == g.CL and g.parts * g.PC == g.CL
        assert (g.SH - 1) * g.SEG < g.NH - 1 <= g.SH * g.SEG if g.NH > 1 else g.SH == 0
        assert g.per_base * g.PC == g.kWin * g.kEnt  # one lane per PC entries of a full-width window
        assert g.table_bytes == 64 * sum(g.ent(w) for w in range(g.kWin))
        assert g.base(g.kWin - 1) + g.ent(g.kWin - 1) == g.words // 16
    g29, g21 = tg.tabgeom(29), tg.tabgeom(21)
    assert g29.widths == [29] * 5 + [28] * 4 and round(g29.table_bytes / 1e9) == 120
    assert g21.widths == [22] * 5 + [21] * 7 and round(g21.table_bytes / 1e9, 2) == 1.14
    assert round(tg.tabgeom(22).table_bytes / 1e9, 2) == 1.61
    assert round(tg.tabgeom(24).table_bytes / 1e9, 1) == 5.9
    assert round(tg.tabgeom(16).table_bytes / 2 ** 20) == 34
    assert (g29.CL, g29.NH, g29.PC, g29.parts) == (1 << 14, 1 << 14, 256, 64)
    g8 = tg.tabgeom(8)
    assert (g8.CL, g8.NH, g8.SEG, g8.SL, g8.SH, g8.PC, g8.parts) == (128, 1, 64, 2, 0, 128, 1)
    g12 = tg.tabgeom(12)
    assert (g12.CL, g12.NH, g12.SEG, g12.SH) == (256, 8, 64, 1)
    assert (tg.tabgeom(16).NH, tg.tabgeom(16).SH) == (128, 2)
    assert tg.tabgeom(20).parts == 4
    # launches of build_tables_w
    assert len(tg.slices(29, 1)) == 36 and len(tg.slices(26, 1)) == 5 and len(tg.slices(24, 1)) == 2
    assert tg.slices(24, 1) == [(0, 1 << 18), (1 << 18, 11 * (1 << 15))]
    assert tg.slices(8, 3) == [(0, 99)]
    for code, nb in ((29, 1), (24, 2), (16, 130), (22, 4), (21, 4)):
        sl = tg.slices(code, nb)
        assert sl[0][0] == 0 and sl[-1][1] == nb * tg.tabgeom(code).per_base
        assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(l1 - l0 == tg.SLICE_LANES for l0, l1 in sl[:-1]) and 0 < sl[-1][1] - sl[-1][0] <= tg.SLICE_LANES
    # 130 keys at 16 bits: the one seam falls inside key 120
    (_, l1), = tg.slices(16, 130)[:1]
    assert l1 // tg.tabgeom(16).per_base == 120 and l1 % tg.tabgeom(16).per_base != 0


def test_slice_seam_probes_against_enumeration(monkeypatch):
    """slice_seam_probes' nearest-writing-lane rule against a lane-by-lane walk
    (code 11 has narrow windows; a small slice cap puts seams everywhere)."""
    for cap in (5, 7, 64, 1000):
        monkeypatch.setattr(tg, "SLICE_LANES", cap)
        for code, nb in ((11, 3), (8, 2), (12, 1)):
            sl = tg.slices(code, nb)
            total = nb * tg.tabgeom(code).per_base
            writes = [tg.lane_entries(code, l) for l in range(total)]

            def last_at_or_below(l):
                while writes[l] is None:
                    l -= 1
                (b, win, _, _), ms = writes[l]
                return (b, win, ms[-1])

            def first_at_or_above(l):
                while l < total and writes[l] is None:
                    l += 1
                if l == total:
                    return None
                (b, win, _, _), ms = writes[l]
                return (b, win, ms[0])

            want = []
            for l0, _ in sl[1:]:
                want += [last_at_or_below(l0 - 1), first_at_or_above(l0)]
            want += [first_at_or_above(sl[-1][0]), last_at_or_below(total - 1)]
            want = [p for p in dict.fromkeys(want) if p is not None]
            assert tg.slice_seam_probes(code, nb) == want, (cap, code, nb)
            for b, win, m in want:
                assert 0 <= b < nb and 1 <= m <= tg.tabgeom(code).ent(win)


def test_probe_multiples_name_the_seams():
    g = tg.tabgeom(16)  # CL 256, NH 128, SEG 64
    ms = tg.probe_multiples(16, 0)
    for m in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 64 * 256, 64 * 256 + 1, 65 * 256,
              127 * 256, 127 * 256 + 1, g.kEnt - 1, g.kEnt, g.kEnt // 2):
        assert m in ms
    assert tg.probe_multiples(8, 0) == [1, 2, 3, 63, 64, 65, 66, 127, 128]
    for code in tg.TABLE_WIDTHS:
        for win in range(tg.tabgeom(code).kWin):
            ms = tg.probe_multiples(code, win)
            assert ms == sorted(set(ms)) and ms[0] == 1 and ms[-1] == tg.tabgeom(code).ent(win)
            assert 2 * tg.tabgeom(code).CL in ms or tg.tabgeom(code).NH == 1


@pytest.mark.parametrize("code", tg.TABLE_WIDTHS + (11,))
def test_only_top_window_probes_may_be_missing(code):
    """Every probe has a scalar unless it is -ent(win) (not a digit) or lies in
    the top window; the scalars recode to the digit they were made for."""
    g = tg.tabgeom(code)
    rng = np.random.default_rng(1000 + code)
    got, missing = tg.table_probes(code, rng)
    for win, m, sign in missing:
        assert tg.may_be_missing(code, win, m, sign), (code, win, m, sign)
    want = sum(2 * len(tg.probe_multiples(code, w)) for w in range(g.kWin))
    assert len(got) + len(missing) == want
    # outside the top window exactly the -ent probes are missing
    assert sorted(p for p in missing if p[0] != g.kWin - 1) == [(w, g.ent(w), -1) for w in range(g.kWin - 1)]
    assert any(win == g.kWin - 1 for win, _, _, _ in got)  # the top window is probed where u < n allows
    for win, m, sign, u in got:
        ds = signed_digits(u, g.widths)
        assert 0 < u < tg.N and ds[win][0] == sign * m
        assert all(d != 0 for i, (d, _) in enumerate(ds) if i < g.kWin - 1), (code, win, m, sign)
    lo, hi = tg.digit_range(g.widths[0])
    assert tg.scalar_with_digit(g.widths, 0, lo - 1, rng) is None
    assert tg.scalar_with_digit(g.widths, 0, hi + 1, rng) is None
    assert tg.scalar_with_digit(g.widths, 0, lo, rng) is not None


@pytest.mark.parametrize("code", [8, 11])
def test_every_probe_reads_its_entry(H, oracle_lib, code):  # noqa: F811
    """On the CPU harness's tables (h_build_table_w; another algorithm than the
    device build, the same layout): the pristine tables accept every probe
    signature, and with one bit flipped in entry base(win) + m - 1 of the
    probed table the same signature is rejected -- for the G table (digit in
    u1) and a key table (digit in u2).  Only the flipped entry's own probe is
    checked: the other digits of a signature are random."""
    g = tg.tabgeom(code)
    rng = np.random.default_rng(77 + code)
    gtab = (ctypes.c_uint32 * g.words)()
    qtab = (ctypes.c_uint32 * g.words)()
    d_priv, pub = tg.make_key(rng, oracle_lib)
    assert H.h_build_table_w(None, code, gtab) == 1
    assert H.h_build_table_w(pub.tobytes(), code, qtab) == 1
    probes, _ = tg.table_probes(code, rng)
    checked = 0
    for table in ("G", "key"):
        work = gtab if table == "G" else qtab
        for win, m, sign, u in probes:
            u1, u2 = (u, tg.rand_scalar(rng)) if table == "G" else (tg.rand_scalar(rng), u)
            h, rs = tg.chosen_scalar_sig_key(d_priv, u1, u2, False, oracle_lib)
            h, rs = h.tobytes(), rs.tobytes()
            assert H.h_verify_w(code, h, rs, gtab, qtab, 1) == 1, (table, win, m, sign)
            word = (g.base(win) + m - 1) * 16 + (win + m) % 16
            work[word] ^= 1 << ((3 * m + win) % 32)
            got = H.h_verify_w(code, h, rs, gtab, qtab, 1)
            work[word] ^= 1 << ((3 * m + win) % 32)
            assert got == 0, (table, win, m, sign)
            checked += 1
    assert checked == 2 * len(probes) and checked >= 2 * g.kWin * 2 * 8


def test_probe_signatures_against_both_oracles(oracle_lib):
    """A (29, 21) probe set needs no table on the CPU: every probe signature is
    accepted, every r-flipped twin rejected, by oracle/p256.py and the C oracle."""
    from oracle import p256
    rng = np.random.default_rng(2921)
    d_priv, pub = tg.make_key(rng, oracle_lib)
    qx, qy = int.from_bytes(pub[:32].tobytes(), "big"), int.from_bytes(pub[32:].tobytes(), "big")
    pg, _ = tg.table_probes(29, rng)
    pq, _ = tg.table_probes(21, rng)
    H_, S_, flipped = [], [], []
    for i in range(max(len(pg), len(pq))):
        u1, u2 = pg[i % len(pg)][3], pq[i % len(pq)][3]
        for flip in (False, True):
            h, rs = tg.chosen_scalar_sig_key(d_priv, u1, u2, flip, oracle_lib)
            H_.append(h)
            S_.append(rs)
            flipped.append(flip)
    flipped = np.array(flipped)
    want = tg.oracle_bits(oracle_lib, np.stack(H_), np.stack(S_), np.zeros(len(H_), np.uint32), pub[None, :])
    assert (want == ~flipped).all()
    for i in range(0, len(H_)):
        rs = S_[i].tobytes()
        ok = p256.verify(H_[i].tobytes(), int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big"), qx, qy)
        assert ok == (not flipped[i]), i
