"""Input families for the field-arithmetic tests: the limb types of rows.h,
fes.h and fe29.h as boxes, and the families that drive every limb to its type
bound (tests/test_rowfield.py on the CPU model, tests/test_gpu_field_probe.py
on the device).  Limb vectors are numpy int64 arrays of shape (n, 9), signed.

Also the per-call generators tests/test_algo_cpu.py has always used (rand_s,
rand_d, rand_l_type and their helpers), unchanged; tests/fieldops_cases.py
draws a share of every S-, D- and L-type operand from them.
"""
from __future__ import annotations

import ctypes

import numpy as np

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
R = 1 << 261
RINV = pow(R, -1, P)
RINV_N = pow(R, -1, N)
M29 = (1 << 29) - 1

M_BOUND = int(1.172 * 2 ** 256)
L_BOUND = int(2.344 * 2 ** 256)
N_BOUND = 2 ** 256 + 2 ** 237
S_BOUND = int(2 ** 257.5)
D_BOUND = int(2 ** 258.5)


# ---- the per-call generators of tests/test_algo_cpu.py ---------------------------
def limbs(v):
    return (ctypes.c_uint32 * 9)(*[(v >> (29 * i)) & M29 for i in range(9)])


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def rand_l_type(rng):
    """A lazily-added (L-type) input: limbs < 2^30, value < 2.344 * 2^256."""
    while True:
        l = [int(rng.choice([rng.integers(0, 1 << 30), (1 << 30) - 1, 0, 1 << 29])) for _ in range(9)]
        l[8] = int(rng.integers(0, 1 << 26))
        if val(l) < L_BOUND:
            return (ctypes.c_uint32 * 9)(*l), val(l)


def slimbs(l):
    return (ctypes.c_uint32 * 9)(*[x & 0xFFFFFFFF for x in l])


def sval(l):
    """value of signed 32-bit limbs"""
    return sum((int(x) - (1 << 32) if int(x) & 0x80000000 else int(x)) << (29 * i) for i, x in enumerate(l))


def s_limbs_of(v):
    """S-type limbs of a (possibly negative) value: limbs 0..7 in [0, 2^29), limb 8 the signed rest"""
    l = [(v >> (29 * i)) & M29 for i in range(8)]
    l.append(v >> 232)
    return l


def rand_s(rng, extreme=False):
    if extreme:
        v = int(rng.choice([S_BOUND - 1, -S_BOUND + 1, 0, P - 1, -(P - 1)]))
        l = s_limbs_of(v)
        if v > 0:
            l[:8] = [M29] * 8 if rng.integers(0, 2) else l[:8]
    else:
        v = int.from_bytes(rng.bytes(33), "big") % (2 * S_BOUND) - S_BOUND
        l = s_limbs_of(v)
    while abs(sum(x << (29 * i) for i, x in enumerate(l))) >= S_BOUND:
        l[8] -= 1 if l[8] > 0 else -1
    return l, sum(x << (29 * i) for i, x in enumerate(l))


def rand_d(rng, extreme=False):
    a, va = rand_s(rng, extreme)
    b, vb = rand_s(rng, extreme)
    d = [x - y for x, y in zip(a, b)]
    return d, va - vb


# ---- limb types as boxes -------------------------------------------------------
# name -> ((lo, hi) of limbs 0..7, (lo, hi) of limb 8), inclusive.  A type with
# a value bound B gets the widest top limb t with (t + 1) 2^232 <= B (limbs
# 0..7 at their bound add less than 2^232, or 2^233 for L), so every vector of
# the box is of the type.
def _top(bound, slack=1):
    return bound // (1 << 232) - slack


_S8, _D8 = _top(S_BOUND), _top(D_BOUND)
TYPES = {
    # rows.h
    "PO": ((-32, (1 << 29) + 31), (-(1 << 25), 1 << 25)),  # a product output: [-2^5, 2^29 + 2^5), top to +-2^25
    "PD": ((-(1 << 29) - 63, (1 << 29) + 63), (-(1 << 26), 1 << 26)),  # a difference of two PO
    "XN": ((-4, (1 << 29) + 3), (-(1 << 25), 1 << 25)),  # a row_norm output
    "WA": ((-(1 << 31) + 1, (1 << 31) - 1), (-(1 << 25), 1 << 25)),  # row_mul's widest pair:
    "WB": ((-(1 << 30) + 1, (1 << 30) - 1), (-(1 << 25), 1 << 25)),  # (2^31 - 1)(2^30 - 1) < 2^61
    "E": ((0, M29), (0, (1 << 24) - 1)),  # a table coordinate (row_entry)
    "EY": ((-M29, M29), (-(1 << 24) + 1, (1 << 24) - 1)),  # ... y with its digit's sign
    # fes.h
    "S": ((0, M29), (-_S8, _S8)),
    "D": ((-M29, M29), (-_D8, _D8)),
    # fe29.h
    "M": ((0, M29), (0, _top(M_BOUND))),
    "NT": ((0, M29), (0, _top(N_BOUND))),
    "L": ((0, (1 << 30) - 1), (0, _top(L_BOUND, 3))),
    # fmont_lane: a < 2^257, b < 2^261, limbs < 2^29
    "FA": ((0, M29), (0, (1 << 25) - 1)),
    "FB": ((0, M29), (0, M29)),
}
VALUE_BOUND = {"S": S_BOUND, "D": D_BOUND, "M": M_BOUND, "NT": N_BOUND, "L": L_BOUND, "FA": 1 << 257, "FB": 1 << 261}


def box(typ):
    (lo, hi), (tlo, thi) = TYPES[typ]
    return np.array([lo] * 8 + [tlo], np.int64), np.array([hi] * 8 + [thi], np.int64)


def values(x):
    """Python integers of limb vectors (n, 9) (or row values (n, 16): lanes past 8 hold 0)"""
    x = np.asarray(x, np.int64)
    return [sum(int(v) << (29 * i) for i, v in enumerate(r[:9])) for r in x.reshape(-1, x.shape[-1])]


def in_type(x, typ):
    lo, hi = box(typ)
    ok = bool(((x >= lo) & (x <= hi)).all())
    if ok and typ in VALUE_BOUND:
        b = VALUE_BOUND[typ]
        ok = all((abs(v) < b) for v in values(x))
    return ok


def random_family(rng, typ, n):
    """iii: limbs uniform in the type's box"""
    lo, hi = box(typ)
    return rng.integers(lo, hi + 1, (n, 9), dtype=np.int64)


N_FIXED = 22  # the deterministic head of bound_family


def bound_family(rng, typ, n):
    """i: every limb at the type's upper bound, at its lower bound, each limb
    position alone at either bound among random ones, then per-limb choices
    among {upper, lower, 0, +-1, random}."""
    assert n >= N_FIXED
    lo, hi = box(typ)
    out = random_family(rng, typ, n)
    out[0], out[1] = hi, lo
    out[2], out[3] = hi, lo
    out[2, 8], out[3, 8] = lo[8], hi[8]
    for k in range(9):
        out[4 + 2 * k, k] = hi[k]
        out[5 + 2 * k, k] = lo[k]
    m = n - N_FIXED
    pick = rng.integers(0, 6, (m, 9))
    one = np.minimum(np.ones(9, np.int64), hi)
    neg = np.maximum(-np.ones(9, np.int64), lo)
    tail = out[N_FIXED:]
    for code, v in ((0, hi), (1, lo), (2, np.zeros(9, np.int64)), (3, one), (4, neg)):
        tail[...] = np.where(pick == code, np.clip(v, lo, hi), tail)
    return out


SPECIAL_VALUES = ([0, 1, -1, P, P - 1, P + 1, R % P, 2 ** 256 - 1] + [k * P for k in range(-5, 6) if k not in (0, 1)])


def write_value(v, typ, rng=None):
    """ii: limbs of `typ` whose value is v (mod p when v itself does not fit the
    type: an unsigned type takes v mod p).  With rng and a signed type wider
    than S, the limb-wise difference of two S-type vectors (v + t) - t."""
    (lo, hi), (tlo, thi) = TYPES[typ]
    if tlo >= 0 and v < 0:
        v %= P
    if typ in ("E", "EY") and not -(1 << 256) < v < (1 << 256):
        v %= P
    if rng is not None and lo <= -M29:
        t = int.from_bytes(rng.bytes(31), "big")
        l = [a - b for a, b in zip(s_limbs_of(v + t), s_limbs_of(t))]
    elif lo < 0 or v >= 0:
        l = s_limbs_of(v)
    else:
        l = s_limbs_of(v % P)
    x = np.array(l, np.int64)
    if not in_type(x[None], typ):  # (k p past an unsigned type's value bound)
        x = np.array(s_limbs_of(v % P), np.int64)
    assert in_type(x[None], typ), (typ, v)
    return x


def special_family(typ, rng=None):
    return np.stack([write_value(v, typ, rng) for v in SPECIAL_VALUES])


def family(rng, typ, n):
    """n vectors of `typ`: the specials (plain, and as differences where the
    type allows), the bound family, the rest random"""
    sp = [special_family(typ)]
    (lo, hi), _ = TYPES[typ]
    if lo <= -M29:
        sp.append(special_family(typ, rng))
    sp = np.concatenate(sp)
    nb = max(N_FIXED, (n - len(sp)) // 2)
    parts = [bound_family(rng, typ, nb), sp]
    rest = n - nb - len(sp)
    assert rest >= 0, (typ, n)
    parts.append(random_family(rng, typ, rest))
    return np.concatenate(parts)


def to_rows(x):
    """(..., 9) limb vectors -> (..., 16) row values (lanes 9..15 hold 0)"""
    x = np.asarray(x, np.int64)
    out = np.zeros(x.shape[:-1] + (16,), np.int64)
    out[..., :9] = x
    return out


def uniform_wave(x):
    """(n, 9) -> (n, 4, 16): the same value in every row of a wave"""
    return np.repeat(to_rows(x)[:, None, :], 4, axis=1)


def shuffled_waves(rng, x):
    """(4 w, 9) -> (w, 4, 16) in a shuffled order: the four rows of a wave carry
    four different cases, extremes beside specials and random ones"""
    assert len(x) % 4 == 0
    return to_rows(x[rng.permutation(len(x))]).reshape(-1, 4, 16)


# ---- curve points in Montgomery XYZZ ---------------------------------------------
def mont(v):
    return v * R % P


def curve_points(n, seed=7):
    """n distinct affine points k G, (k + 1) G, .. (plain integers)"""
    from oracle import p256
    pt = p256.scalar_mult(0xC0FFEE + seed, p256.G)
    out = []
    for _ in range(n):
        out.append(pt)
        pt = p256.point_add(pt, p256.G)
    return out


def xyzz_of(pt, z, neg=False):
    """Montgomery XYZZ values (x Z^2, y Z^3, Z^2, Z^3) R mod p of an affine point"""
    x, y = pt
    if neg:
        y = P - y
    zz, zzz = z * z % P, z * z * z % P
    return [mont(x * zz % P), mont(y * zzz % P), mont(zz), mont(zzz)]


def xyzz_limbs(vals, types, rng):
    """four values -> (4, 9) limbs, coordinate k written in types[k]"""
    return np.stack([write_value(v, t, rng if t in ("PD", "D") else None) for v, t in zip(vals, types)])


def entry_words(x, y):
    """a table entry: x, y (< 2^256) as 8 + 8 little-endian words"""
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [(y >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def entry_table():
    """vi: coordinates 0, 1, p - 1, 2^256 - 1 and single bits at every limb seam
    (bits 29 k - 1 and 29 k, limb 8's bit 232 at word 7 among them), as x and as
    y beside a different x; (ents, 16) uint32"""
    coords = [0, 1, P - 1, 2 ** 256 - 1] + [1 << b for k in range(1, 9) for b in (29 * k - 1, 29 * k)] + [1 << 255]
    ent = [entry_words(c, coords[(i + 5) % len(coords)] ^ (1 << 255)) for i, c in enumerate(coords)]
    ent += [entry_words(coords[(i + 3) % len(coords)], c) for i, c in enumerate(coords)]
    return np.array(ent, np.uint32)


# ---- the cases of each operation (shared by the CPU and the GPU test) ------------
ROW_MUL_PAIRS = [("PO", "PO"), ("PO", "PD"), ("PD", "PD"), ("XN", "PD"), ("E", "EY"), ("WA", "WB"), ("WB", "WA")]


def row_mul_cases(rng, n_waves):
    """(a, b) of (n_waves, 4, 16) and, per product, its pair of types: every
    pair's families meet index by index (upper x upper, lower x lower) and once
    more shifted by one (upper x lower); the four rows of a wave carry four
    different products"""
    n = 4 * n_waves
    m = (n // (2 * len(ROW_MUL_PAIRS))) & ~1
    fa, fb, ty = [], [], []
    for ta, tb in ROW_MUL_PAIRS:
        a, b = family(rng, ta, m), family(rng, tb, m)
        fa += [a, a]
        fb += [b, np.roll(b, 1, axis=0)]
        ty += [(ta, tb)] * (2 * m)
    rest = n - 2 * m * len(ROW_MUL_PAIRS)
    fa.append(random_family(rng, "PO", rest))
    fb.append(random_family(rng, "PD", rest))
    ty += [("PO", "PD")] * rest
    a, b = np.concatenate(fa), np.concatenate(fb)
    perm = rng.permutation(n)
    return to_rows(a[perm]).reshape(-1, 4, 16), to_rows(b[perm]).reshape(-1, 4, 16), [ty[i] for i in perm]


ROW_POINT = ("PO", "PD", "PO", "PO")  # X, Y, ZZ, ZZZ of a row-schedule XYZZ point
QUAD_POINT = ("S", "D", "S", "S")  # ... of a quad-schedule one


def _point_set(rng, pts, types, neg=False, z=None):
    return np.stack([xyzz_limbs(xyzz_of(pt, int(rng.integers(2, 1 << 62)) ** 4 % P if z is None else z, neg), types,
                                rng) for pt in pts])


def add_cases(rng, n, types, rm_type, n_curve=256):
    """A, B of (n, 4, 9), rm (n, 9) and labels: i-iii on every coordinate (not
    curve points: the formulas are algebraic), then iv: real curve points with
    random Z, P == Q and P == -Q under different Z, an operand whose ZZ (and
    ZZZ) is already 0 (mod p, in several representations)"""
    k = n_curve // 4
    nf = n - 4 * k
    A = np.stack([family(rng, t, nf) for t in types], axis=1)
    B = np.stack([family(rng, t, nf)[rng.permutation(nf)] for t in types], axis=1)
    B[:N_FIXED] = np.stack([bound_family(rng, t, N_FIXED) for t in types], axis=1)  # bounds meet bounds
    up, low = B[0].copy(), B[1].copy()  # A's head: upper, lower, upper (top lower), lower (top upper)
    B[1], B[2], B[3] = up, low, low  # upper x upper, lower x upper, upper x lower, lower x lower
    lab = ["family"] * nf
    if k == 0:
        return A, B, family(rng, rm_type, n)[rng.permutation(n)], lab
    pts = curve_points(2 * k, 11)
    pa, pb = pts[:k], pts[k:]
    A = np.concatenate([A, _point_set(rng, pa, types), _point_set(rng, pa, types), _point_set(rng, pa, types),
                        _point_set(rng, pa, types)])
    zero = _point_set(rng, pb, types)
    for i in range(k):  # ZZ == ZZZ == 0 (mod p): 0, p, -p, 2p, ...
        zero[i, 2] = write_value((i % 5 - 2) * P, types[2])
        zero[i, 3] = write_value(((i // 5) % 5 - 2) * P, types[3])
    B = np.concatenate([B, _point_set(rng, pb, types), _point_set(rng, pa, types), _point_set(rng, pa, types, True),
                        zero])
    lab += ["curve"] * k + ["double"] * k + ["cancel"] * k + ["zz0"] * k
    rm = family(rng, rm_type, n)[rng.permutation(n)]
    return A, B, rm, lab


def mmadd_cases(rng, n):
    """gx, gy, qx, qy of (n, 9): table coordinates (E) and y with its digit's
    sign (EY); curve points among them, and qx == gx (P == 0)"""
    k = n // 8
    out = [family(rng, t, n - 3 * k)[rng.permutation(n - 3 * k)] for t in ("E", "EY", "E", "EY")]
    pts = curve_points(2 * k, 13)
    g, q = pts[:k], pts[k:]

    def aff(ps, neg):
        xs = np.stack([write_value(mont(x), "E") for x, _ in ps])
        ys = np.stack([write_value(mont(y), "E") for _, y in ps])
        return xs, np.where(neg[:, None], -ys, ys)

    sg, sq = rng.integers(0, 2, k).astype(bool), rng.integers(0, 2, k).astype(bool)
    for (ga, qa) in ((aff(g, sg), aff(q, sq)), (aff(g, sg), aff(g, sg)), (aff(g, sg), aff(g, ~sg))):
        for i, v in enumerate((ga[0], ga[1], qa[0], qa[1])):
            out[i] = np.concatenate([out[i], v])
    return out, ["family"] * (n - 3 * k) + ["curve"] * k + ["double"] * k + ["cancel"] * k


def chain_leaves(rng, chains, types):
    """iv: 16 leaves per chain for a 4-level tree (outputs feed inputs); in
    chain c >= 2 leaf 1 is leaf 0 again (c even) or its negative (c odd), under
    another Z: ZZ == 0 must come out at level 1 and stay 0 to the top"""
    pts = curve_points(16 * chains, 17)
    leaves = _point_set(rng, pts, types).reshape(chains, 16, 4, 9)
    for c in range(2, chains):
        leaves[c, 1] = _point_set(rng, [pts[16 * c]], types, neg=bool(c & 1))[0]
    return leaves, pts


def check_cases(rng, n, types, rz_type):
    """v: A, B (n, 4, 9), rz (n, 9) and the expected (verdict, exc): the true r
    (accept), r ^ 2 (reject), P == 0 (exc), r ZZ1 ZZ2 == 0 (exc; through ZZ2 and
    through rz), in turn"""
    from oracle import p256
    k = n // 6
    pts = curve_points(2 * n, 19)
    A, B, rz, want = [], [], [], []
    for i in range(n):
        pa, pb = pts[2 * i], pts[2 * i + 1]
        kind = i % 6 if i < 6 * k else 0
        z1, z2 = (int(rng.integers(2, 1 << 62)) ** 4 % P for _ in range(2))
        r = p256.point_add(pa, pb)[0]
        ok, exc = True, False
        if kind == 1:
            r, ok = r ^ 2, False
        a = xyzz_limbs(xyzz_of(pa, z1), types, rng)
        if kind in (2, 3):  # P == 0: B is A again, or -A
            pb, exc = pa, True
        b = xyzz_limbs(xyzz_of(pb, z2, neg=kind == 3), types, rng)
        rzv = mont(r * z1 * z1 % P)
        if kind == 4:
            b[2], exc = write_value((i % 5 - 2) * P, types[2]), True
        if kind == 5:
            rzv, exc = (i % 3 - 1) * P, True
        A.append(a)
        B.append(b)
        rz.append(write_value(rzv, rz_type))
        want.append((ok, exc))
    return np.stack(A), np.stack(B), np.stack(rz), want


def plain(x):
    """the field elements of Montgomery-form limb vectors"""
    return [v * RINV % P for v in values(x)]


def add_formula(a, b, rm=None):
    """add-2008-s on plain field elements a, b = (x, y, zz, zzz): the sum and r ZZ3"""
    u1, u2, s1, s2 = a[0] * b[2], b[0] * a[2], a[1] * b[3], b[1] * a[3]
    p, r = u2 - u1, s2 - s1
    pp = p * p
    ppp, q = p * pp, u1 * pp
    x3 = r * r - ppp - 2 * q
    out = [x3 % P, (r * (q - x3) - s1 * ppp) % P, a[2] * b[2] * pp % P, a[3] * b[3] * ppp % P]
    return out, (None if rm is None else rm * out[2] % P)


def mmadd_formula(gx, gy, qx, qy):
    """mmadd-2008-s on plain affine coordinates"""
    p, r = qx - gx, qy - gy
    pp = p * p
    ppp, q = p * pp, gx * pp
    x3 = r * r - ppp - 2 * q
    return [x3 % P, (r * (q - x3) - gy * ppp) % P, pp % P, ppp % P]


def check_formula(a, b, rz):
    """the fused last level on plain values: (X3 == r ZZ3, exc)"""
    u1, u2, s1, s2 = a[0] * b[2], b[0] * a[2], a[1] * b[3], b[1] * a[3]
    p, r = u2 - u1, s2 - s1
    rz12 = rz * b[2]
    return (r * r - p * p * (p + 2 * u1 + rz12)) % P == 0, p % P == 0 or rz12 % P == 0
