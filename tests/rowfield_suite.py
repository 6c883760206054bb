"""Every rows.h operation's cases (the families of rowfield_cases.py) with what the
limb-exact model of rowfield.py computes for them: the expectations that
tests/test_rowfield.py checks against Python integers and that
tests/test_gpu_field_probe.py compares the device with."""
from __future__ import annotations

import functools

import numpy as np

import rowfield_cases as rc
from rowfield import RowModel


def _wave4(pt):
    """(n, 4, 9) points -> four (n, 4, 16) wave values, the same in every row"""
    return [rc.uniform_wave(pt[:, k]) for k in range(4)]


@functools.lru_cache(maxsize=None)
def row_suite(n_waves, chains=64):
    """The cases of every rows.h operation at `n_waves` waves each, and what
    one RowModel (suite["model"], whose stats then cover them all) computes
    for them.  Built once per size; the tests must not modify it."""
    rng = np.random.default_rng(0x0F1E1D + n_waves)
    m = RowModel()
    s = {"model": m}
    a, b, ty = rc.row_mul_cases(rng, n_waves)
    s["row_mul"] = dict(a=a, b=b, types=ty, out=m.row_mul(a, b))
    # row_norm: any limbs of |l| < 2^31 -- WA, and differences and triple sums of outputs
    x = np.concatenate([rc.family(rng, "WA", 2 * n_waves), rc.family(rng, "PD", n_waves),
                        3 * rc.family(rng, "PO", n_waves)])
    x = rc.shuffled_waves(rng, x)
    s["row_norm"] = dict(x=x, out=m.row_norm(x))
    A, B, rm, lab = rc.add_cases(rng, n_waves, rc.ROW_POINT, "PO")
    out, rz = m.xyzz_add_rows(_wave4(A), _wave4(B), rc.uniform_wave(rm))
    s["add"] = dict(A=A, B=B, rm=rm, labels=lab, out=out, rz=rz)
    (gx, gy, qx, qy), lab = rc.mmadd_cases(rng, 2 * n_waves)  # two additions per wave
    pair = lambda v: np.repeat(rc.to_rows(v).reshape(-1, 2, 16), 2, axis=1)  # noqa: E731
    ins = [pair(v) for v in (gx, gy, qx, qy)]
    s["mmadd"] = dict(ins=ins, labels=lab, out=m.mmadd_pairs(*ins))
    # iv: a 4-level tree per chain, the model's outputs feeding the next level
    leaves, pts = rc.chain_leaves(rng, chains, rc.ROW_POINT)
    rmc = rc.family(rng, "E", chains)
    level, cur = [], [rc.uniform_wave(leaves[:, :, k].reshape(-1, 9)) for k in range(4)]
    for lv in range(4):
        n = cur[0].shape[0] // 2
        Ain, Bin = [v[0::2] for v in cur], [v[1::2] for v in cur]
        rml = rc.uniform_wave(np.repeat(rmc, n // chains, axis=0))
        out, rz = m.xyzz_add_rows(Ain, Bin, rml)
        level.append(dict(A=Ain, B=Bin, rm=rml, out=out, rz=rz))
        cur = out
    s["chain"] = dict(levels=level, points=pts, chains=chains)
    A, B, rz, want = rc.check_cases(rng, n_waves, rc.ROW_POINT, "PO")
    # ... and i-iii on every coordinate of the fused check as well
    A2, B2, rz2, _ = rc.add_cases(rng, n_waves, rc.ROW_POINT, "PO", n_curve=0)
    A, B, rz = np.concatenate([A, A2]), np.concatenate([B, B2]), np.concatenate([rz, rz2])
    ok, exc = m.xyzz_add_check_rows(_wave4(A), _wave4(B), rc.uniform_wave(rz))
    s["check"] = dict(A=A, B=B, rz=rz, want=want, ok=ok, exc=exc)
    # row_is_zero / row_to_fe: k p in every type, values beside them, and the families
    z = np.concatenate([rc.family(rng, t, n_waves // 2) for t in ("PO", "PD")])
    z = rc.uniform_wave(z[rng.permutation(len(z))])
    z[:, 1:] = z[rng.permutation(len(z)), 1:]  # rows 1..3 carry other values: only row 0 counts
    s["zero"] = dict(x=z, out=m.row_is_zero(z))
    return s
