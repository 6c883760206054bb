"""The row layout of simple_pbft_amd/csrc/rows.h restated limb for limb, and
the quad schedule of verify_kernels.h composed from the CPU harness's products.

rows.h cannot be compiled for the CPU (DPP moves, permlane swaps), so this is
its twin: the same additions, shifts and masks in the same order, on exact
integers.  A row value is an int64 array (..., 16): lane j holds limb j as the
signed 32-bit number the VGPR holds, lanes 9..15 hold 0.  A wave is (n, 4, 16):
n cases, four rows.  Everything is vectorised over the cases; int64 is exact
here because the model asserts, before anything could wrap, the very bounds
that rows.h states (a column stays below 2^61.2 and a stored limb inside
int32, so no sum below leaves int64).

RowModel asserts the header's claims on every call and keeps running maxima
(RowModel.stats):
  * every stored limb fits int32;
  * max|a_i| max|b_j| < 2^61 for every product, every column below 2^61.2;
  * product limbs 0..7 in [-2^5, 2^29 + 2^5), row_norm's in [-2^2, 2^29 + 2^2);
  * w of the fused check has limbs < 3 2^29 + 2^6;
  * lanes 9..15 stay 0.
"""
from __future__ import annotations

import ctypes

import numpy as np

from rowfield_cases import M29, P

PL = np.array([(P >> (29 * i)) & M29 for i in range(9)] + [0] * 7, np.int64)
ONE_P = [((1 << 261) % P >> (29 * i)) & M29 for i in range(9)]
COL_BOUND = int(2 ** 61.2)
PROD_BOUND = 1 << 61
W_BOUND = 3 * (1 << 29) + (1 << 6)
I32_LO, I32_HI = -(1 << 31), (1 << 31) - 1


class RowBoundError(AssertionError):
    """a bound of rows.h's header does not hold"""


def _next(x):  # row_next: lane j <- lane j + 1 of its row, 0 past it
    out = np.zeros_like(x)
    out[..., :-1] = x[..., 1:]
    return out


def _prev(x):  # row_prev: lane j <- lane j - 1 of its row, 0 before it
    out = np.zeros_like(x)
    out[..., 1:] = x[..., :-1]
    return out


_L8 = np.arange(16) == 8


class RowModel:
    """norm_x3 / w_sum: the two mutants of tests/test_rowfield.py's teeth --
    X3 without its row_norm, and w formed as P + 2 U1 + r ZZ12."""

    def __init__(self, norm_x3=True, w_sum=True):
        self.norm_x3, self.w_sum = norm_x3, w_sum
        self.stats = {"prod": 0, "col": 0, "carry_min": 0, "carry_max": 0, "limb_min": 0, "limb_max": 0,
                      "norm_min": 0, "norm_max": 0, "w_max": 0, "stored": 0, "products": 0}

    def _up(self, key, v, f=max):
        self.stats[key] = f(self.stats[key], int(v))

    def reg(self, x, what="value"):
        """a value as a VGPR holds it: every limb inside int32, lanes 9..15 zero"""
        x = np.asarray(x, np.int64)
        lo, hi = int(x.min()), int(x.max())
        self._up("stored", max(-lo, hi))
        if lo < I32_LO or hi > I32_HI:
            raise RowBoundError("%s leaves int32: limbs in [%d, %d]" % (what, lo, hi))
        if x[..., 9:].any():
            raise RowBoundError("%s: lanes 9..15 are not zero" % what)
        return x

    # ---- rows.h ----------------------------------------------------------------
    def row_mul(self, a, b):
        a, b = self.reg(a, "row_mul a"), self.reg(b, "row_mul b")
        a, b = np.broadcast_arrays(a, b)
        pm = np.abs(a).max(axis=-1).astype(object) * np.abs(b).max(axis=-1).astype(object)
        self._up("prod", pm.max())
        if pm.max() >= PROD_BOUND:
            raise RowBoundError("max|a_i| max|b_j| = 2^%.2f" % np.log2(float(pm.max())))
        self.stats["products"] += int(np.prod(a.shape[:-1]))
        t = np.zeros(a.shape, np.int64)
        for i in range(9):
            t = t + a[..., i:i + 1] * b
            q = t[..., 0:1] & M29  # -p^-1 = 1 (mod 2^29)
            t = t + q * PL
            col = int(np.abs(t).max())
            self._up("col", col)
            if col >= COL_BOUND:
                raise RowBoundError("a column reaches 2^%.2f" % np.log2(col))
            assert not (t[..., 0] & M29).any()  # the column is divisible now
            t = (t >> 29) + _next(t & M29)
        if int(t[..., 8].min()) < I32_LO or int(t[..., 8].max()) > I32_HI:
            raise RowBoundError("row_mul: limb 8 leaves int32")
        lo = np.where(_L8, t, t & M29)  # lane 8 keeps its whole limb ...
        hi = np.where(_L8, 0, t >> 29)  # ... and carries nothing up
        self._up("carry_min", hi.min(), min)
        self._up("carry_max", hi.max())
        out = self.reg(lo + _prev(hi), "row_mul's output")
        self._up("limb_min", out[..., :8].min(), min)
        self._up("limb_max", out[..., :8].max())
        if int(out[..., :8].min()) < -(1 << 5) or int(out[..., :8].max()) >= (1 << 29) + (1 << 5):
            raise RowBoundError("row_mul: output limbs leave [-2^5, 2^29 + 2^5)")
        return out

    def row_norm(self, x):
        x = self.reg(x, "row_norm's input")
        lo = np.where(_L8, x, x & M29)
        hi = np.where(_L8, 0, x >> 29)
        out = self.reg(lo + _prev(hi), "row_norm's output")
        self._up("norm_min", out[..., :8].min(), min)
        self._up("norm_max", out[..., :8].max())
        if int(out[..., :8].min()) < -4 or int(out[..., :8].max()) >= (1 << 29) + 4:
            raise RowBoundError("row_norm: output limbs leave [-2^2, 2^29 + 2^2)")
        return out

    @staticmethod
    def gather4(x):
        """g[r] = row r's x, in every row"""
        return [np.broadcast_to(x[:, r:r + 1, :], x.shape) for r in range(4)]

    @staticmethod
    def sel4(v0, v1, v2, v3):
        """row r takes v_r"""
        vs = [v0, v1, v2, v3]
        ref = next(v for v in vs if not isinstance(v, int))
        vs = [np.zeros_like(ref) + v if isinstance(v, int) else v for v in vs]
        return np.stack([vs[r][:, r, :] for r in range(4)], axis=1)

    def x3_step(self, RR, PPP, Q):
        """X3 = R^2 - PPP - 2Q renormalised, and Q - X3 (both must fit int32)"""
        X3 = self.reg(RR - PPP - self.reg(Q << 1, "2 Q"), "R^2 - PPP - 2 Q")
        if self.norm_x3:
            X3 = self.row_norm(X3)
        return X3, self.reg(Q - X3, "Q - X3")

    def xyzz_add_rows(self, A, B, rm):
        """A, B: (x, y, zz, zzz) of (n, 4, 16); returns (x, y, zz, zzz), rz"""
        s, g4 = self.sel4, self.gather4
        A = [self.reg(v) for v in A]
        B = [self.reg(v) for v in B]
        g = g4(self.row_mul(s(A[0], B[0], A[1], B[1]), s(B[2], A[2], B[3], A[3])))  # U1, U2, S1, S2
        U1, S1 = g[0], g[2]
        Pd, Rd = self.reg(g[1] - g[0], "P"), self.reg(g[3] - g[2], "R")
        g = g4(self.row_mul(s(Pd, Rd, A[2], A[3]), s(Pd, Rd, B[2], B[3])))  # PP, R^2, ZZ1 ZZ2, ZZZ1 ZZZ2
        PP, RR, Z12, ZZZ12 = g
        g = g4(self.row_mul(s(Pd, U1, Z12, 0), PP))  # PPP, Q = U1 PP, ZZ3
        PPP, Q, ZZ3 = g[0], g[1], g[2]
        X3, t = self.x3_step(RR, PPP, Q)
        g = g4(self.row_mul(s(Rd, S1, ZZZ12, self.reg(rm)), s(t, PPP, PPP, ZZ3)))  # R (Q - X3), S1 PPP, ZZZ3, r ZZ3
        return [X3, self.reg(g[0] - g[1], "Y3"), ZZ3, g[2]], g[3]

    def mmadd_pairs(self, gx, gy, qx, qy):
        """rows 0, 1 hold window A's values, rows 2, 3 window B's"""
        g4 = self.gather4
        odd = (np.arange(4) & 1).astype(bool)[None, :, None]
        pb = (np.arange(4) >= 2)[None, :, None]
        p, rr = self.reg(qx - gx, "p"), self.reg(qy - gy, "r")
        m = np.where(odd, rr, p)
        g = g4(self.row_mul(m, m))  # PP, R^2 of each pair
        PP, R2 = np.where(pb, g[2], g[0]), np.where(pb, g[3], g[1])
        g = g4(self.row_mul(np.where(odd, gx, p), PP))  # PPP, Q = X1 PP
        PPP, Q = np.where(pb, g[2], g[0]), np.where(pb, g[3], g[1])
        X3, t = self.x3_step(R2, PPP, Q)
        g = g4(self.row_mul(np.where(odd, gy, rr), np.where(odd, PPP, t)))  # R (Q - X3), Y1 PPP
        return [X3, self.reg(np.where(pb, g[2] - g[3], g[0] - g[1]), "Y3"), PP, PPP]

    @staticmethod
    def row_to_fe(x):
        """the value of row 0 as nine limbs (n, 9)"""
        return x[:, 0, :9]

    def fs_norm(self, d):
        """fes.h fs_norm on (n, 9): one signed carry pass, every step inside int32"""
        d = np.array(d, np.int64)
        for i in range(8):
            d[:, i + 1] += d[:, i] >> 29
            d[:, i] &= M29
            self.reg(to16(d), "fs_norm")
        return d

    def fs_is_zero(self, d):
        """fes.h fs_is_zero on (n, 9): fe_fold_carry, then the digits against p's"""
        d = np.array(d, np.int64)
        top = (d[:, 8] - 4) >> 24
        d[:, 8] -= top << 24
        d[:, 0] += top
        d[:, 3] -= top << 9
        d[:, 6] -= top << 18
        d[:, 7] += top << 21
        self.reg(to16(d), "fe_fold_carry")
        for i in range(8):
            d[:, i + 1] += d[:, i] >> 29
            d[:, i] &= M29
        self.reg(to16(d), "fe_fold_carry")
        return (d == PL[:9]).all(axis=1)

    def row_is_zero(self, x):
        return self.fs_is_zero(self.fs_norm(self.row_to_fe(self.reg(x))))

    def xyzz_add_check_rows(self, A, B, rz):
        """returns (verdict, exc), bool arrays (n,)"""
        s, g4 = self.sel4, self.gather4
        A = [self.reg(v) for v in A]
        B = [self.reg(v) for v in B]
        g = g4(self.row_mul(s(A[0], B[0], A[1], B[1]), s(B[2], A[2], B[3], A[3])))  # U1, U2, S1, S2
        U1, U2 = g[0], g[1]
        Pd, Rd = self.reg(g[1] - g[0], "P"), self.reg(g[3] - g[2], "R")
        g = g4(self.row_mul(s(Pd, Rd, self.reg(rz), 0), s(Pd, Rd, B[2], 0)))  # PP, R^2, r ZZ1 ZZ2
        PP, R2, rz12 = g[0], g[1], g[2]
        if self.w_sum:
            w = self.reg(self.reg(U1 + U2, "U1 + U2") + rz12, "w")
        else:
            w = self.reg(self.reg(Pd + self.reg(U1 << 1, "2 U1"), "P + 2 U1") + rz12, "w")
        self._up("w_max", np.abs(w[..., :8]).max())
        if int(w[..., :8].max()) >= W_BOUND or int(w[..., :8].min()) < -W_BOUND:
            raise RowBoundError("w: limbs reach %d" % int(np.abs(w[..., :8]).max()))
        odd = (np.arange(4) & 1).astype(bool)[None, :, None]
        g = g4(self.row_mul(np.where(odd, Pd, PP), np.where(odd, rz12, w)))  # PP w; P r ZZ1 ZZ2
        a = self.row_to_fe(self.reg(R2 - g[0], "R^2 - PP w"))
        b = self.row_to_fe(g[1])
        return self.fs_is_zero(self.fs_norm(a)), self.fs_is_zero(self.fs_norm(b))


def to16(d):
    out = np.zeros(d.shape[:-1] + (16,), np.int64)
    out[..., :d.shape[-1]] = d
    return out


def alignbit(hi, lo, sh):
    """v_alignbit_b32: the low 32 bits of (hi:lo) >> sh"""
    return (((hi << 32) | lo) >> sh) & 0xFFFFFFFF


def row_entry(table, d, L):
    """verify_kernels.h row_entry at window 0: lane L's (x, y) limbs of digit d's
    entry, from the two words its limb spans (the sign is the caller's)"""
    idx = (-d if d < 0 else d) - 1
    p = [int(w) for w in table[0 if idx < 0 else idx]]
    Lc = L if L < 9 else 0
    bit = 29 * Lc
    wi, sh = bit >> 5, bit & 31
    wj = wi + 1 if wi < 7 else wi
    m = M29 if L < 9 else 0
    x = alignbit(p[wj] if wi < 7 else 0, p[wi], sh) & m
    y = alignbit(p[8 + wj] if wi < 7 else 0, p[8 + wi], sh) & m
    return x, y


# ---- the quad schedule, composed from the CPU harness ------------------------------
class QuadModel:
    """quad_mul / quad_mmadd_xyzz / quad_xyzz_add / quad_xyzz_add_check of
    verify_kernels.h on (n, 9) uint32 limb arrays: the harness's fs_mul and
    fs_norm (libalgo_harness.so, hb_fs_mul / hb_fs_helpers) in the order the
    device code calls them; the limb-wise steps in uint32, which wraps as the
    device does."""

    def __init__(self, lib):
        self.lib = lib

    def _call(self, name, inp, nout):
        inp = np.ascontiguousarray(inp, np.uint32)
        out = np.zeros((len(inp), nout), np.uint32)
        getattr(self.lib, "hb_" + name)(ctypes.c_void_p(inp.ctypes.data), ctypes.c_void_p(out.ctypes.data), len(inp))
        return out

    def mul(self, a, b):
        return self._call("fs_mul", np.concatenate([a, b], axis=1), 18)[:, :9]

    def norm(self, a):
        return self._call("fs_helpers", a, 19)[:, :9]

    def is_zero(self, a):
        return self._call("fs_helpers", a, 19)[:, 18] != 0

    def mmadd(self, gx, gy, qx, qy, rm):
        p, rr = qx - gx, qy - gy
        pp, r2 = self.mul(p, p), self.mul(rr, rr)
        ppp, qq = self.mul(p, pp), self.mul(gx, pp)
        x3 = self.norm(r2 - ppp - (qq << 1))
        t = qq - x3
        a, b, rz = self.mul(rr, t), self.mul(gy, ppp), self.mul(rm, pp)
        return [x3, a - b, pp, ppp], rz

    def add(self, Pt, Qt, rm, qinf):
        u1, u2 = self.mul(Pt[0], Qt[2]), self.mul(Qt[0], Pt[2])
        s1, s2 = self.mul(Pt[1], Qt[3]), self.mul(Qt[1], Pt[3])
        p, rr = u2 - u1, s2 - s1
        pp, r2 = self.mul(p, p), self.mul(rr, rr)
        zz12, zzz12 = self.mul(Pt[2], Qt[2]), self.mul(Pt[3], Qt[3])
        ppp, qq, zz3 = self.mul(p, pp), self.mul(u1, pp), self.mul(zz12, pp)
        x3 = self.norm(r2 - ppp - (qq << 1))
        t = qq - x3
        zsel = np.where(np.asarray(qinf, bool)[:, None], Pt[2], zz3)
        a, b = self.mul(rr, t), self.mul(s1, ppp)
        return [x3, a - b, zz3, self.mul(zzz12, ppp)], self.mul(rm, zsel)

    def add_check(self, Pt, Qt, rz):
        u1, u2 = self.mul(Pt[0], Qt[2]), self.mul(Qt[0], Pt[2])
        s1, s2 = self.mul(Pt[1], Qt[3]), self.mul(Qt[1], Pt[3])
        p, rr = u2 - u1, s2 - s1
        exc = self.is_zero(p)
        pp, r2, rz12 = self.mul(p, p), self.mul(rr, rr), self.mul(rz, Qt[2])
        exc = exc | self.is_zero(rz12)
        w = self.norm((u1 << 1) + rz12) + p
        return self.is_zero(r2 - self.mul(pp, w)), exc
