"""The device table build's geometry, restated, and signatures that read a
chosen entry of a chosen table (tests/test_tabgeom.py, tests/test_gpu_tables.py).

Test infrastructure only.  The comb tables are built on the device by
k_tab_bases / k_tab_small / k_tab_entries (p256_kernels.hip, TabGeom): entry
m B_i of window i is H_hi + L_lo with m = hi CL + lo + 1, the H rows cut into
segments of SEG multiples (phase 2), the entries into chunks of PC (phase 3,
one lane each), phase 3 launched in slices of at most 2^18 lanes that run
across windows and bases.  The CPU harness builds its tables with other code
(p256_algo.h build_table_serial), so the device build is only checked through
what a verify reads -- and a verify reads entry |d| - 1 of window i for the
signed digit d of u1 (G table) or u2 (key table).  Since (e, r, s) are free
inputs, a signature with chosen (u1, u2) puts any digit in any window:

  * `tabgeom` restates CombGeom / TabGeom for a geometry code;
  * `lane_entries` / `slices` restate which multiples a phase-3 lane writes
    and how build_tables_w cuts the lanes into launches;
  * `probe_multiples` / `slice_seam_probes` list the multiples at the seams of
    that build (first / last of a segment, chunk, H row, window, launch; the
    one doubling entry m = 2 CL);
  * `scalar_with_digit` makes a scalar with a given digit in a given window,
    `chosen_scalar_sig_key` a signature whose verify recomputes given
    (u1, u2) under a key with a known private scalar.

Expected accept bits never come from here: the callers ask the oracle."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import window_widths  # noqa: E402
from conftest import signed_digits  # noqa: E402

N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551

# every table width the device instantiates (kernels.h PBFTV_TABLE_WIDTHS); the CPU harness adds the mixed code 11
TABLE_WIDTHS = (8, 12, 16, 20, 21, 22, 24, 26, 29)
SLICE_LANES = 1 << 18  # table_scratch_sizes: phase-3 lanes per launch


class TabGeom:
    """CombGeom<code> and TabGeom<code>, by the same rules."""

    def __init__(self, code: int):
        self.code = code
        self.widths = window_widths(code)
        self.kW = self.widths[0]
        self.kWin = len(self.widths)
        self.kEnt = 1 << (self.kW - 1)
        self._ent = [1 << (w - 1) for w in self.widths]
        self._bit = [sum(self.widths[:i]) for i in range(self.kWin)]
        self._base = [sum(self._ent[:i]) for i in range(self.kWin)]
        self.words = sum(self._ent) * 16
        self.table_bytes = self.words * 4
        # L rows: (lo + 1) B_i, lo < CL; H rows: hi (CL B_i), 1 <= hi < NH
        if self.kEnt < 256:
            self.CL = self.kEnt
        else:
            self.CL = 256 if self.kW <= 16 else 1 << (self.kW // 2)
        self.NH = self.kEnt // self.CL
        # phase 2: lanes of SEG consecutive multiples (SL segments of L, SH of H)
        self.SEG = min(self.CL, 64)
        self.SL = self.CL // self.SEG
        self.SH = (self.NH - 1 + self.SEG - 1) // self.SEG if self.NH > 1 else 0
        # phase 3: lanes of PC entries sharing one H
        self.PC = min(self.CL, 256)
        self.parts = self.CL // self.PC
        self.per_base = self.kWin * self.NH * self.parts

    def ent(self, win: int) -> int:
        return self._ent[win]

    def bit(self, win: int) -> int:
        return self._bit[win]

    def base(self, win: int) -> int:
        return self._base[win]


@functools.lru_cache(maxsize=None)
def tabgeom(code: int) -> TabGeom:
    return TabGeom(code)


def lane_entries(code: int, lane: int):
    """Phase-3 lane `lane` of a build (k_tab_entries): ((b, win, hi, part),
    range of the multiples m it writes into window win of base b), or None for
    a lane past the entries of a narrow top window."""
    g = tabgeom(code)
    b, rem = divmod(lane, g.per_base)
    win, rem = divmod(rem, g.NH * g.parts)
    hi, part = divmod(rem, g.parts)
    if hi * g.CL >= g.ent(win):
        return None
    m0 = hi * g.CL + part * g.PC + 1
    return (b, win, hi, part), range(m0, m0 + g.PC)


def slices(code: int, nb: int) -> list:
    """The [lane0, lane1) phase-3 launches of build_tables_w for nb bases."""
    total = nb * tabgeom(code).per_base
    step = min(total, SLICE_LANES)
    return [(l0, min(l0 + step, total)) for l0 in range(0, total, step)]


def probe_multiples(code: int, win: int) -> list:
    """The multiples m = |digit| at the seams of window `win`'s build."""
    g = tabgeom(code)
    CL, SEG, PC, NH, ent = g.CL, g.SEG, g.PC, g.NH, g.ent(win)
    ms = [1, 2, 3]
    ms += [SEG - 1, SEG, SEG + 1, SEG + 2]
    ms += [PC - 1, PC, PC + 1]
    ms += [CL - 1, CL, CL + 1, CL + 2]
    ms += [2 * CL - 1, 2 * CL, 2 * CL + 1]       # the doubling entry and its neighbours
    ms += [3 * CL - 1, 3 * CL, 3 * CL + 1]       # the same place one H row up: no doubling
    ms += [SEG * CL, SEG * CL + 1, (SEG + 1) * CL, (SEG + 1) * CL + 1, (SEG + 2) * CL]  # H segment seam
    ms += [(NH - 1) * CL, (NH - 1) * CL + 1, ent - 1, ent]
    ms += [ent // 2 - 1, ent // 2, ent // 2 + 1]
    return sorted({m for m in ms if 1 <= m <= ent})


def _lane(g: TabGeom, b: int, win: int, hi: int, part: int) -> int:
    return ((b * g.kWin + win) * g.NH + hi) * g.parts + part


def _writer_at_or_below(code: int, lane: int):
    """The nearest lane <= `lane` that writes entries."""
    g = tabgeom(code)
    if lane_entries(code, lane) is None:  # past a narrow window: back to that window's last chunk
        b, rem = divmod(lane, g.per_base)
        win = rem // (g.NH * g.parts)
        lane = _lane(g, b, win, g.ent(win) // g.CL - 1, g.parts - 1)
    return lane


def _writer_at_or_above(code: int, lane: int, total: int):
    """The nearest lane >= `lane` (and < total) that writes entries, or None."""
    g = tabgeom(code)
    if lane_entries(code, lane) is None:  # past a narrow window: on to the next window's first chunk
        b, rem = divmod(lane, g.per_base)
        win = rem // (g.NH * g.parts)
        lane = _lane(g, b, win + 1, 0, 0) if win + 1 < g.kWin else (b + 1) * g.per_base
    return lane if lane < total else None


def slice_seam_probes(code: int, nb: int) -> list:
    """(b, win, m) at the launch seams of a build of nb bases: for every
    boundary lane0 between two launches the last multiple written by lane
    lane0 - 1 and the first written by lane lane0 (the nearest writing lane on
    that side, where the lane itself writes nothing), and the first and last
    multiples written by the final (shorter) launch."""
    sl = slices(code, nb)
    total = sl[-1][1]

    def last_of(lane):
        (b, win, _, _), ms = lane_entries(code, _writer_at_or_below(code, lane))
        return (b, win, ms[-1])

    def first_of(lane):
        lane = _writer_at_or_above(code, lane, total)
        if lane is None:
            return None
        (b, win, _, _), ms = lane_entries(code, lane)
        return (b, win, ms[0])

    out = []
    for l0, _ in sl[1:]:
        out += [last_of(l0 - 1), first_of(l0)]
    out += [first_of(sl[-1][0]), last_of(total - 1)]
    seen, uniq = set(), []
    for p in out:
        if p is not None and p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def digit_range(width: int):
    """signed_digit_w's range for a window of `width` bits."""
    return -((1 << (width - 1)) - 1), 1 << (width - 1)


def _rand_below(rng, bound: int) -> int:
    """Uniform in [0, bound) from a numpy Generator."""
    return int.from_bytes(rng.bytes((bound.bit_length() + 7) // 8 + 8), "big") % bound


def _rand_digit(rng, width: int) -> int:
    lo, hi = digit_range(width)
    d = lo + _rand_below(rng, hi - lo)  # lo .. hi - 1
    return d if d < 0 else d + 1        # skip 0


def scalar_with_digit(widths, win: int, d: int, rng, tries: int = 20):
    """A scalar u in (0, n) whose signed recoding over `widths`
    (conftest.signed_digits) has digit d in window `win`, every other digit
    random and non-zero where possible; None when there is none.

    The digit ranges are complete residue systems, so the recoding of an
    integer is unique: u has digit d in `win` exactly when u = v + k M with
    v = d 2^bit(win) + (the windows below, any digits) and M = 2^bit(win + 1).
    The windows below are drawn as digits; the windows above follow from a
    random k that keeps 0 < u < n (k = 0 in the top window)."""
    nwin = len(widths)
    bits = [sum(widths[:i]) for i in range(nwin)]
    lo_d, hi_d = digit_range(widths[win])
    if not lo_d <= d <= hi_d:
        return None
    top = win == nwin - 1
    M = 1 << (bits[win] + widths[win])

    def finish(lower):
        v = (d << bits[win]) + sum(x << bits[i] for i, x in enumerate(lower))
        if top:
            return v if 0 < v < N else None
        kmin, kmax = (-v) // M + 1, (N - 1 - v) // M  # 0 < v + k M < n
        if kmin > kmax:
            return None
        return v + (kmin + _rand_below(rng, kmax - kmin + 1)) * M

    best, best_zeros = None, None
    for _ in range(tries):
        u = finish([_rand_digit(rng, widths[i]) for i in range(win)])
        if u is None:
            continue
        zeros = sum(1 for i, (x, _) in enumerate(signed_digits(u, widths)) if x == 0 and i != win and i != nwin - 1)
        if best is None or zeros < best_zeros:
            best, best_zeros = u, zeros
        if zeros == 0:
            break
    if best is None:  # the extremes of the windows below decide whether any u exists
        for pick in (0, 1):
            best = finish([digit_range(widths[i])[pick] for i in range(win)])
            if best is not None:
                break
    if best is None:
        return None
    ds = signed_digits(best, widths)
    assert ds[win][0] == d and sum(x << b for x, b in ds) == best and 0 < best < N
    return best


def table_probes(code: int, rng):
    """Every (win, m, sign) of probe_multiples over all windows of a table,
    each with a scalar that has digit sign * m there.  Returns (realised:
    [(win, m, sign, u)], missing: [(win, m, sign)]); see `may_be_missing` for
    what may be missing."""
    g = tabgeom(code)
    got, missing = [], []
    for win in range(g.kWin):
        for m in probe_multiples(code, win):
            for sign in (1, -1):
                u = scalar_with_digit(g.widths, win, sign * m, rng)
                if u is None:
                    missing.append((win, m, sign))
                else:
                    got.append((win, m, sign, u))
    return got, missing


def may_be_missing(code: int, win: int, m: int, sign: int) -> bool:
    """A probe has no scalar only as -ent(win) (not a digit) or in the top
    window (u < n bounds the digit)."""
    g = tabgeom(code)
    return (sign < 0 and m == g.ent(win)) or win == g.kWin - 1


def chosen_scalar_sig_key(d_priv: int, u1: int, u2: int, flip_r: bool, oracle_lib):
    """conftest.chosen_scalar_sig for the key d_priv G: R = (u1 + u2 d) G by
    the C oracle, r = x(R) mod n (1 when R is infinity), s = r / u2, e = u1 s,
    so the verify recomputes exactly (u1, u2).  Returns (hash, r||s)."""
    k = (u1 + u2 * d_priv) % N
    r = 1
    if k:
        out = np.zeros(64, np.uint8)
        assert oracle_lib.oracle_p256_pubkey(k.to_bytes(32, "big"), out.ctypes.data) == 1
        r = int.from_bytes(out[:32].tobytes(), "big") % N
    s = r * pow(u2, -1, N) % N
    e = u1 * s % N
    if flip_r:
        r ^= 2
    return (np.frombuffer(e.to_bytes(32, "big"), np.uint8),
            np.frombuffer(r.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint8))


def rand_scalar(rng) -> int:
    return 1 + _rand_below(rng, N - 1)


def make_key(rng, oracle_lib):
    """(private scalar, public key X||Y as 64 bytes) from the C oracle."""
    d = rand_scalar(rng)
    out = np.zeros(64, np.uint8)
    assert oracle_lib.oracle_p256_pubkey(d.to_bytes(32, "big"), out.ctypes.data) == 1
    return d, out


def oracle_bits(oracle_lib, H, S, K, keys) -> np.ndarray:
    """oracle_ecdsa_p256_verify_batch over the batch: the expected accept bits."""
    H, S = np.ascontiguousarray(H, np.uint8), np.ascontiguousarray(S, np.uint8)
    K, keys = np.ascontiguousarray(K, np.uint32), np.ascontiguousarray(keys, np.uint8)
    n = len(K)
    bm = np.zeros((n + 7) // 8, np.uint8)
    oracle_lib.oracle_ecdsa_p256_verify_batch(H.ctypes.data, S.ctypes.data, K.ctypes.data, n, keys.ctypes.data,
                                              len(keys), bm.ctypes.data, 8)
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)
