"""Python restatements of the device's inversion mod n (verify_kernels.h
inv_mod_n_wave), shared by tests/test_algo_cpu.py, tests/scalar_cases.py and
tests/test_scalar_cases.py.  Exact integers throughout.

  _divsteps30_var      safegcd.h divsteps30_var on 32-bit words (the C++ form
                       that divsteps30_scalar's comment calls its reference).
  divsteps30_states    the CONTROL FLOW of divsteps30_scalar's assembly: the
                       register roles, the four sign/role states S0..S3, the
                       fast "goes on and swaps" branch, the rare path's three
                       outcomes and the four exit blocks, instruction by
                       instruction on 32-bit registers.  It asserts on every
                       call that it returns what _divsteps30_var returns, and
                       records the events it went through.
  _inv_wave            the lane-limb scheme: one list entry per lane, 30-bit
                       signed limbs re-centred after every batch, divsteps on
                       the low limbs only, centred md / me, e = R mod n at the
                       start; it asserts what the kernel's int32 / int64
                       arithmetic relies on.
  inv_stats            the same values on whole integers (no limbs, no bound
                       assertions): fast enough for searches over tens of
                       thousands of inputs.  tests/test_scalar_cases.py checks
                       it against _inv_wave.

This is a restatement of the kernel text, not the kernel: what it proves is
that the scheme is right and which inputs reach which of its paths; the GPU
tests (tests/test_gpu_scalar_seams.py) then feed those inputs to the device."""
from __future__ import annotations

_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
_M30 = (1 << 30) - 1
_M32 = 0xFFFFFFFF
_NINV30 = 0x11FF43B1  # verify_kernels.h kNInv30

STATES = (0, 1, 2, 3)
PATHS = ("fast-swap", "rare-swap", "rare-elim", "exit")
TERMS = ("e1", "i", "cap")


def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _i32(x):
    assert -(1 << 31) <= x < (1 << 31)
    return x


def _divsteps30_var(eta, f, g):
    """safegcd.h divsteps30_var on 32-bit words."""
    u, v, q, r, i = 1, 0, 0, 1, 30
    f &= 0xFFFFFFFF
    g &= 0xFFFFFFFF
    while True:
        gg = (g | (0xFFFFFFFF << i)) & 0xFFFFFFFF
        z = (gg & -gg).bit_length() - 1
        g >>= z
        u = (u << z) & 0xFFFFFFFF
        v = (v << z) & 0xFFFFFFFF
        eta -= z
        i -= z
        if i == 0:
            return eta, _s32(u), _s32(v), _s32(q), _s32(r)
        if eta < 0:
            eta = -eta
            f, g, u, q, v, r = g, -f & 0xFFFFFFFF, q, -u & 0xFFFFFFFF, r, -v & 0xFFFFFFFF
        m = (0xFFFFFFFF >> (32 - min(eta + 1, i))) & 63
        w = (f * g * ((f * f - 2) & 0xFFFFFFFF)) & m
        g, q, r = (g + f * w) & 0xFFFFFFFF, (q + u * w) & 0xFFFFFFFF, (r + v * w) & 0xFFFFFFFF


# register roles of the assembly: copy A = (f, g, u, v, q, r), copy B = (g, f, q, r, u, v)
_ROLES_A = ("f", "g", "u", "v", "q", "r")
_ROLES_B = ("g", "f", "q", "r", "u", "v")


def divsteps30_states(eta, f, g, events=None):
    """divsteps30_scalar's assembly, block by block (verify_kernels.h
    PBFTV_DS_STEP / SWAPIN / ELIM / RARE and the exit blocks .Lx0 .. .Lx3).

    State s: S0 = A(+,+), S1 = B(+,-), S2 = A(-,-), S3 = B(-,+).  A STEP in an
    even state works on (g, u, v), in an odd one on (f, q, r); a swap goes from
    s to s + 1 mod 4, exchanges the roles and recomputes nfi from the new f row
    (negated in the odd states); an elimination adds in the even states and
    subtracts in the odd ones.

    events (a set, optional) receives (state of the STEP, path, width, terms):
    path one of PATHS; width = min(e1, i, 6) of the elimination that follows
    (None for "exit"); terms = which of "e1", "i", "cap" equal that width.

    Returns (eta, u, v, q, r) and asserts that _divsteps30_var returns the same."""
    R = {"f": f & _M32, "g": g & _M32, "u": 1, "v": 0, "q": 0, "r": 1}
    st = {"e1": (eta + 1) & _M32, "i": 30, "nfi": ((f & _M32) * ((f * f - 2) & _M32)) & _M32}

    def step(s, first=False):  # PBFTV_DS_STEP: SCC at its end = "goes on AND swaps"
        # e1 < 1 only at a batch's first STEP (in S0): the rare path's swap is dead code in S1..S3
        assert first or _s32(st["e1"]) >= 1
        G, U, V = ("g", "u", "v") if s % 2 == 0 else ("f", "q", "r")
        z = (R[G] & -R[G]).bit_length() - 1 if R[G] else _M32  # s_ff1_i32_b32: -1 for 0
        goes_on = z < st["i"]                                  # s_min_u32's SCC
        z = min(z, st["i"])
        k = st["e1"] if goes_on else _M32                      # s_cselect_b32
        R[G] >>= z
        R[U] = (R[U] << z) & _M32
        R[V] = (R[V] << z) & _M32
        st["e1"] = (st["e1"] - z) & _M32
        st["i"] -= z
        return k <= z                                          # s_cmp_le_u32 k, z

    def swapin(s):  # PBFTV_DS_SWAPIN on entering state s
        F = "g" if s % 2 else "f"
        st["e1"] = (2 - st["e1"]) & _M32
        w = (R[F] * R[F]) & _M32
        w = (2 - w) & _M32 if s % 2 else (w - 2) & _M32        # PBFTV_DS_NFI_NEG / _POS
        st["nfi"] = (w * R[F]) & _M32

    def elim(s):  # PBFTV_DS_ELIM in state s; returns (width, terms)
        F, G, U, V, Q, Rr = _ROLES_A if s % 2 == 0 else _ROLES_B
        sign = 1 if s % 2 == 0 else -1                         # s_add_u32 / s_sub_u32
        w = (R[G] * st["nfi"]) & _M32
        m = min(st["e1"], st["i"], 6)                          # two s_min_u32
        terms = tuple(t for t, val in (("e1", st["e1"]), ("i", st["i"]), ("cap", 6)) if val == m)
        w &= (1 << m) - 1                                      # s_bfm_b32 m, 0
        R[G] = (R[G] + sign * R[F] * w) & _M32
        R[Q] = (R[Q] + sign * R[U] * w) & _M32
        R[Rr] = (R[Rr] + sign * R[V] * w) & _M32
        return m, terms

    def note(s, path, wt=(None, ())):
        if events is not None:
            events.add((s, path, wt[0], wt[1]))

    s = 0
    fast = step(0, first=True)
    while True:
        if fast:                                # .Ll<s+1>: swap, eliminate, .Le<s+1>
            s0, s = s, (s + 1) % 4
            swapin(s)
            note(s0, "fast-swap", elim(s))
        elif st["i"] == 0:                      # .Lr<s>: s_cmp_eq_u32 i, 0 -> .Lx<s>
            note(s, "exit")
            break
        elif _s32(st["e1"]) < 1:                # s_cmp_lt_i32 e1, 1 -> .Ll<s+1>
            s0, s = s, (s + 1) % 4
            swapin(s)
            note(s0, "rare-swap", elim(s))
        else:                                   # elimination without a swap -> .Le<s>
            note(s, "rare-elim", elim(s))
        fast = step(s)
    u, v, q, r = R["u"], R["v"], R["q"], R["r"]
    if s == 1:    # .Lx1  B(+,-): u = q', v = r', q = -u', r = -v'
        u, v, q, r = q, r, -u & _M32, -v & _M32
    elif s == 2:  # .Lx2  A(-,-)
        u, v, q, r = -u & _M32, -v & _M32, -q & _M32, -r & _M32
    elif s == 3:  # .Lx3  B(-,+): u = -q', v = -r', q = u', r = v'
        u, v, q, r = -q & _M32, -r & _M32, u, v
    out = (_s32(st["e1"]) - 1, _s32(u), _s32(v), _s32(q), _s32(r))
    assert out == _divsteps30_var(eta, f, g), (eta, hex(f & _M32), hex(g & _M32), out)
    return out


def _center(limbs):
    cs = [((x + (1 << 29)) >> 30) if L < 8 else 0 for L, x in enumerate(limbs)]
    return [_i32(x - (c << 30) + (cs[L - 1] if L else 0)) for L, (x, c) in enumerate(zip(limbs, cs))]


def _shift30(cols):
    for p in cols:
        assert abs(p) < (1 << 61)  # int64 with room: |u A + v B + md n_L| < 2^60.x
    lo = [((p & _M30) ^ (1 << 29)) - (1 << 29) for p in cols]
    assert lo[0] == 0  # the batch's matrix makes the low limb vanish
    hi = [_i32((p - l) >> 30) for p, l in zip(cols, lo)]
    return [_i32(hi[L] + (lo[L + 1] if L < 8 else 0)) for L in range(9)]


def _limbs30(x):
    return [(x >> (30 * L)) & _M30 for L in range(8)] + [x >> 240]


def _value(limbs):
    return sum(v << (30 * L) for L, v in enumerate(limbs))


def _center30(x):
    """verify_kernels.h center30 of a 32-bit word"""
    return _s32(x << 2) >> 2


def _inv_wave(x, stats=None, events=None):
    """The lane-limb scheme of inv_mod_n_wave.  Returns (D, batches) with D =
    R x^-1 + k n in (0, 2^261).  stats (a dict, optional) receives "batches",
    "max_eta" (the largest |eta| between batches) and "max_d" (the largest of
    |d| / n and |e| / n after any batch, a float).  With events (a set), every
    batch runs divsteps30_states, which checks itself against _divsteps30_var."""
    n_l = _limbs30(_N)
    f, g = _center(n_l), _center(_limbs30(x))
    d, e = [0] * 9, _center(_limbs30((1 << 261) % _N))
    eta, batches, max_eta, max_d = -1, 0, 1, 0
    for _ in range(25):
        batches += 1
        if events is not None:
            eta, u, v, q, r = divsteps30_states(eta, f[0], g[0], events)
        else:
            eta, u, v, q, r = _divsteps30_var(eta, f[0], g[0])
        d0, e0 = d[0] & 0xFFFFFFFF, e[0] & 0xFFFFFFFF
        md = _s32((-((u * d0 + v * e0) * 0x11FF43B1)) << 2) >> 2   # center30(0 - c nInv30)
        me = _s32((-((q * d0 + r * e0) * 0x11FF43B1)) << 2) >> 2
        f, g = (_center(_shift30([u * a + v * b for a, b in zip(f, g)])),
                _center(_shift30([q * a + r * b for a, b in zip(f, g)])))
        d, e = (_center(_shift30([u * a + v * b + md * nl for a, b, nl in zip(d, e, n_l)])),
                _center(_shift30([q * a + r * b + me * nl for a, b, nl in zip(d, e, n_l)])))
        for limbs in (f, g, d, e):
            assert all(abs(t) <= (1 << 29) + 2 for t in limbs[:8])
        assert abs(_value(d)) < 13.5 * _N and abs(_value(e)) < 13.5 * _N
        max_eta = max(max_eta, abs(eta))
        max_d = max(max_d, abs(_value(d)), abs(_value(e)))
        if not any(g):
            break
    fv = _value(f)
    assert fv in (1, -1)
    pos = (f[0] + (f[1] << 30)) & 0xFFFFFFFF == 1  # the kernel's sign test
    assert pos == (fv == 1)
    D = (_value(d) if pos else -_value(d)) + 16 * _N
    assert 0 < D < (1 << 261)
    if stats is not None:
        stats.update(batches=batches, max_eta=max_eta, max_d=max_d / _N)
    return D, batches


def inv_stats(x):
    """(D, batches, max_eta, max_d) of _inv_wave(x) computed on whole integers:
    f, g, d, e are the values the limbs stand for (re-centring changes no value,
    md / me depend on d, e mod 2^30 only).  For searches."""
    f, g, d, e = _N, x, 0, (1 << 261) % _N
    eta, batches, max_eta, max_d = -1, 0, 1, 0
    for _ in range(25):
        batches += 1
        eta, u, v, q, r = _divsteps30_var(eta, f, g)
        md = _center30(-((u * d + v * e) * _NINV30))
        me = _center30(-((q * d + r * e) * _NINV30))
        f, g = (u * f + v * g) >> 30, (q * f + r * g) >> 30
        d, e = (u * d + v * e + md * _N) >> 30, (q * d + r * e + me * _N) >> 30
        max_eta = max(max_eta, abs(eta))
        max_d = max(max_d, abs(d), abs(e))
        if g == 0:
            break
    assert f in (1, -1)
    return f * d + 16 * _N, batches, max_eta, max_d / _N
