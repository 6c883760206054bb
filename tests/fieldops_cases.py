"""The cases of tests/cpp/field_ops.h's wrappers (fes.h, fe29.h, p256_algo.h and
sec1.h, one operation each): their inputs from the families of
rowfield_cases.py, and what their outputs must be as Python integers.  The CPU
test runs them through the g++ build (tests/test_rowfield.py), the GPU test
through the device build as well (tests/test_gpu_field_probe.py)."""
from __future__ import annotations

import ctypes

import numpy as np

import rowfield_cases as rc
from rowfield_cases import N, P, RINV_N


def run(lib, name, inp, out_words):
    """one entry point (fp_NAME of the probe, hb_NAME of the harness) over the cases of inp (n, words)"""
    inp = np.ascontiguousarray(inp, np.uint32)
    n = inp.shape[0]
    out = np.zeros((n, out_words), np.uint32)
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int if name.startswith("fp_") else None
    err = fn(ctypes.c_void_p(inp.ctypes.data), ctypes.c_void_p(out.ctypes.data), ctypes.c_int(n))
    assert not err, "%s: hipError_t %s" % (name, err)
    return out


def op_words(lib, prefix, name):
    """(words in, words out) per case of a field_ops.h wrapper, from the library's own table"""
    i, o = ctypes.c_int(), ctypes.c_int()
    fn = getattr(lib, prefix + "words")
    fn.restype = ctypes.c_int
    assert fn(name.encode(), ctypes.byref(i), ctypes.byref(o)) == 0, name
    return i.value, o.value


def run_op(lib, prefix, name, inp):
    """a field_ops.h wrapper (hb_NAME of the harness, fp_NAME of the probe): the
    buffers take their widths from the library that writes them"""
    iw, ow = op_words(lib, prefix, name)
    assert inp.shape[1] == iw, (name, inp.shape, iw)
    return run(lib, prefix + name, inp, ow)


def u32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def s32(x):
    return np.asarray(x, np.uint32).astype(np.int32).astype(np.int64)


def _mix(rng, x, k):
    """an operand's cases: the head keeps the bounds in place (upper meets upper,
    lower meets lower, and for a later operand upper meets lower), the rest is shuffled"""
    x = x.copy()
    if k:
        x[2], x[3] = x[1].copy(), x[0].copy()
    x[4:] = x[4 + rng.permutation(len(x) - 4)]
    return x


N_GEN = 96  # per part of type S, D or L: cases from the generators test_algo_cpu.py draws from
GENERATORS = {"S": rc.rand_s, "D": rc.rand_d, "L": lambda rng, ext: rc.rand_l_type(rng)}


def _generated(rng, t):
    """rand_s / rand_d (every third one extreme) / rand_l_type, as limb vectors"""
    return np.array([[int(v) for v in GENERATORS[t](rng, i % 3 == 0)[0]] for i in range(N_GEN)], np.int64)


def _operand(rng, types, n, k):
    m = n // len(types)
    parts = [rc.family(rng, t, m if j else n - m * (len(types) - 1)) for j, t in enumerate(types)]
    for t, part in zip(types, parts):
        if t in GENERATORS:
            part[-N_GEN:] = _generated(rng, t)
    head = parts[k % len(parts)][:4].copy()
    x = np.concatenate(parts)
    x[:4] = head
    return _mix(rng, x, k)


SD, MNL = ("S", "D"), ("M", "NT", "L")


def _madd_flip(x, y, zz, zzz, x2, y2):
    u2, s2 = x2 * zz, y2 * zzz
    p, r = u2 - x, s2 - y
    pp = p * p
    ppp, q = p * pp, x * pp
    x3 = r * r - ppp - 2 * q
    return [x3, r * (x3 - q) + y * ppp, zz * pp, zzz * ppp]


def _aff_aff(x0, y0, x1, y1, flip):
    e = -y0 if flip else y0
    d, p = y1 - e, x1 - x0
    pp = p * p
    ppp, q = p * pp, x0 * pp
    x3 = d * d - ppp - 2 * q
    return [x3, d * (x3 - q) + e * ppp, pp, ppp]


def _last_d(x, y, zz, zzz, x2, y2, rz):
    u2, s2 = x2 * zz, y2 * zzz
    p, rr = u2 - x, s2 - y
    return [rr * rr - p * p * (u2 + x + rz)]


# name -> (operand types, extra words, what the output field elements are, on plain values)
C_OPS = {
    "fs_mul": ([SD, SD], 0, lambda a, b: [a * b] * 2),
    "fs_sqr": ([SD], 0, lambda a: [a * a] * 2),
    "fs_mul2_add": ([SD, SD, ("D",), ("S",)], 0, lambda a, b, c, d: [a * b + c * d] * 2),
    "fs_sqr_sub2": ([("D",), ("S",), ("S",)], 0, lambda a, b, c: [a * a - b - 2 * c] * 3),
    "fs_sqr_mul_add": ([("D",), ("S",), ("S",)], 0, lambda a, b, c: [a * a + b * c]),
    "fs_mul_x2": ([SD, SD, SD, SD], 0, lambda a, b, c, d: [a * b, c * d] * 3),
    "fs_sqr_sub2_mul": ([("D",), ("S",), ("S",), SD, SD], 0, lambda a, b, c, e, f: [a * a - b - 2 * c, e * f] * 3),
    "fs_mul2_add_mul": ([SD, SD, ("D",), ("S",), SD, SD], 0, lambda a, b, c, d, e, f: [a * b + c * d, e * f] * 2),
    "fs_helpers": ([SD], 0, None),
    "xyzz_madd_s_flip": ([("S",), ("S",), ("S",), ("S",), ("E",), ("EY",)], 0, _madd_flip),
    "xyzz_aff_aff_s": ([("E",), ("E",), ("E",), ("E",)], 1, _aff_aff),
    "xyzz_last_s": ([("S",), ("S",), ("S",), ("S",), ("E",), ("EY",), ("S",)], 0, _last_d),
    "fe_mul": ([MNL, MNL], 0, lambda a, b: [a * b]),
    "fe_sqr": ([MNL], 0, lambda a: [a * a]),
    "fe_mul2_add": ([("M", "NT"), ("M", "NT"), MNL, ("M", "NT")], 0, lambda a, b, c, d: [a * b + c * d]),
    "fe_sub": ([MNL, MNL], 0, None),
    "fe_mul_small": ([("M", "NT")], 1, None),
    "fe_canon": ([("M", "NT")], 0, None),
    "fn_mul": ([("FA",), ("FA",)], 0, None),
    "fe_sqrt_p": ([MNL], 0, None),
    "entry_to_fe_cneg": ([], 17, None),
}
def c_inputs(name, rng, n):
    types, extra, _ = C_OPS[name]
    ops = [_operand(rng, t, n, k) for k, t in enumerate(types)]
    ex = None
    if name == "fs_helpers":  # fs_norm takes any limbs |l| < 2^31 - 2^3; the zero test needs multiples of p
        ops[0][n // 2:] = rc.random_family(rng, "S", n - n // 2) * 3 - rc.random_family(rng, "S", n - n // 2)
        for i, k in enumerate(range(-5, 6)):
            for j, t in enumerate(("D", "D", "S")):
                ops[0][32 + 3 * i + j] = rc.write_value(k * P, t, rng if j else None)
    elif name == "xyzz_aff_aff_s":
        ex = rng.integers(0, 2, (n, 1))
    elif name == "fe_mul_small":
        ex = rng.integers(1, 4, (n, 1))
    elif name == "fe_sqrt_p":  # squares, non-squares and 0 (0, p, 2p), Montgomery form, in every type
        for i in range(n // 2):
            s = int.from_bytes(rng.bytes(32), "big") % P
            v = rc.mont(s * s % P) if i % 8 else (i // 8 % 3) * P
            t = MNL[i % 3]
            ops[0][4 + i] = rc.write_value(v + (P if t == "L" and i % 2 else 0), t)
    elif name == "xyzz_last_s":  # accepts among them: curve points, rz = r ZZ1 for the sum's x
        from oracle import p256
        pts = rc.curve_points(128, 23)
        for i in range(64):
            z = int(rng.integers(2, 1 << 62)) ** 4 % P
            pa, pb = pts[2 * i], pts[2 * i + 1]
            r = p256.point_add(pa, pb)[0] ^ (2 if i % 4 == 3 else 0)
            acc = rc.xyzz_of(pa, z)
            vals = acc + [rc.mont(pb[0]), rc.mont(pb[1]) * (-1 if i & 1 else 1), rc.mont(r * z * z % P)]
            if i & 1:
                vals[1] = P - vals[1]  # W = sigma Y with sigma = -1: y2 comes as sigma y2
            for k, v in enumerate(vals):
                ops[k][8 + i] = rc.write_value(v, types[k][0]) if k != 5 else rc.write_value(abs(v), "E") * (
                    -1 if v < 0 else 1)
    elif name == "entry_to_fe_cneg":
        tab = rc.entry_table()
        w = rng.integers(0, 1 << 32, (n, 16), dtype=np.uint64)
        w[:2 * len(tab)] = np.concatenate([tab, tab])
        ex = np.concatenate([w, (np.arange(n) >= len(tab))[:, None] & 1], axis=1)
        ex[2 * len(tab):, 16] = rng.integers(0, 2, n - 2 * len(tab))
    inp = [u32(v) for v in ops] + ([] if ex is None else [np.asarray(ex).astype(np.uint32)])
    return ops, ex, np.concatenate(inp, axis=1)


def _fes(out, k):
    """the k-th field element of each case's output, signed limbs"""
    return s32(out[:, 9 * k:9 * k + 9])


def check_values(name, ops, ex, out):
    """the harness's limbs (which the device's must equal) against Python integers"""
    n = len(out)
    types, _, f = C_OPS[name]
    pl = [rc.plain(v) for v in ops]
    if f is not None:
        nres = len(f(*([1] * len(ops)), *([0] if ex is not None else [])))
        got = [rc.plain(_fes(out, k)) for k in range(nres)]
        for i in range(n):
            args = [p[i] for p in pl] + ([int(ex[i, 0])] if ex is not None else [])
            assert [g[i] for g in got] == [w % P for w in f(*args)], (name, i)
    if name in ("fs_mul", "fs_sqr", "fs_mul2_add", "fs_sqr_mul_add", "fs_mul_x2", "fs_mul2_add_mul"):
        assert int(_fes(out, 0)[:, :8].min()) >= 0 and int(_fes(out, 0)[:, :8].max()) < 1 << 29  # S-type
    if name.startswith("fe_") or name == "fn_mul":
        assert int(out[:, :9].max()) < 1 << 29
    vin = [rc.values(v) for v in ops]
    if name == "fs_helpers":
        assert rc.values(_fes(out, 0)) == vin[0] and int(_fes(out, 0)[:, :8].min()) >= 0
        assert int(_fes(out, 0)[:, :8].max()) < 1 << 29
        half = n // 2  # (the second half is wider than D-type: fs_norm only)
        assert rc.values(_fes(out, 1))[:half] == [v % P for v in vin[0][:half]]
        zero = [v % P == 0 for v in vin[0][:half]]
        assert list(out[:half, 18]) == zero and sum(zero) >= 33
    elif name == "xyzz_last_s":
        d = rc.values(_fes(out, 0))
        assert list(out[:, 9]) == [v % P == 0 for v in d]
        assert list(out[8:72, 9]) == [i % 4 != 3 for i in range(64)]  # the true r accepted, r ^ 2 not
    elif name == "fe_sub":
        assert [v % P for v in rc.values(_fes(out, 0))] == [(a - b) % P for a, b in zip(*vin)]
        assert max(rc.values(_fes(out, 0))) < rc.N_BOUND
    elif name == "fe_mul_small":
        assert [v % P for v in rc.values(_fes(out, 0))] == [a * int(k) % P for a, k in zip(vin[0], ex[:, 0])]
    elif name == "fe_canon":
        assert rc.values(_fes(out, 0)) == [a % P for a in vin[0]]
    elif name == "fn_mul":
        got = rc.values(_fes(out, 0))
        assert [v % N for v in got] == [a * b * RINV_N % N for a, b in zip(*vin)] and max(got) < 1 << 257
    elif name == "fe_sqrt_p":
        y = rc.plain(_fes(out, 0))
        sq = [pow(t, (P - 1) // 2, P) != P - 1 for t in pl[0]]
        assert list(out[:, 9]) == sq and n // 2 < sum(sq) < n and sum(t == 0 for t in pl[0]) >= n // 32
        assert all(r * r % P == t for r, t, s in zip(y, pl[0], sq) if s)
        assert all(r * r % P == P - t for r, t, s in zip(y, pl[0], sq) if not s)  # t^((p+1)/4) all the same
    elif name == "entry_to_fe_cneg":
        x = [sum(int(w) << (32 * i) for i, w in enumerate(e[:8])) for e in ex]
        yv = [sum(int(w) << (32 * i) for i, w in enumerate(e[8:16])) * (-1 if e[16] else 1) for e in ex]
        assert rc.values(_fes(out, 0)) == x and rc.values(_fes(out, 1)) == yv
        assert int(np.abs(_fes(out, 1)).max()) < 1 << 29 and int(out[:, :9].max()) < 1 << 29
