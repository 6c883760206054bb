"""Chosen-scalar signatures under keys whose private scalar nobody knows, for the
verify that carries its key (simple_pbft_amd/csrc/varbase.h, sec1.h,
p256_varbase.hip): tests/test_carried_cases.py (CPU) and
tests/test_gpu_carried_seams.py (GPU) share what this module builds.

The construction.  For ANY point Q and any u1, 0 < u2 < n, let
R = u1 G + u2 Q (oracle/p256.py), r = x(R) mod n, s = r / u2, e = u1 s mod n.
The verifier of (e, r, s) under Q recomputes exactly (u1, u2): a client who
picks (r, s, e) and the key picks every digit of both scalars and every
coordinate the lane's table 1Q .. 8Q is built from.

Four families, each computed once and cached here; every expected bit is the C
oracle's (oracle_ecdsa_p256_verify) and is asserted equal to what the
construction intends:
  ladder      u2 chosen digit by digit (vb_recode, vb_ladder) under >= 3 keys
  G part      u1 chosen window by window (vb_next_gdigit, vb_load_g), with
              doublings and cancellations solved for under keys Q = d G
  key shape   full-length scalars under every key of KEYS (edge coordinates)
  SEC1        compressed keys over a sweep of X (sec1_decompress, fe_sqrt_p)
combined() concatenates them, in natural order and in one seeded permutation.

Two facts the cases rest on.  The comb's 17th window is read by every u1 whose
top 16 bits exceed 0x8000 (the carry out of window 15), about half of all
signatures, not only by u1 >= 0xFFFF8001 << 224; the cases built AT that
window still use such a u1, where g_15 is 0 or -1.  And a built-in meeting
leaves Z == 0 with X == 0 one addition later, so a verifier that took such a
result for a finite point would compare 0 == r * 0 and accept ANY r: every
meeting with a finite R therefore has a twin with another r over the same
scalars (OTHER_R), expected 0.

A case is a row of: hash (32 B), r||s (64 B), key X||Y (64 B), expected bit,
name, rerun (True / False: the exact rerun must / must not run; None: not
pinned), family.  A compressed key without a point is carried as X || 0..0p
with p the prefix's parity bit: wirekey_cases.encode() turns that row into
exactly the compressed key, and as X||Y it is off the curve (y <= 1 is a root
of no X swept here, asserted below)."""
from __future__ import annotations

import numpy as np

import wirekey_cases as wc
from conftest import signed_digits
from oracle import p256

P, N = p256.P, p256.N
G = p256.G
FAMILIES = ("ladder", "gpart", "keyshape", "sec1")
PLAIN, FLIP_R, E_PLUS_N, OTHER_R = "plain", "r ^ 2", "e + n", "r + 1, same scalars"
KIND_PLAIN, KIND_RERUN, KIND_REJECTED_KEY = 0, 1, 2
R261 = pow(2, 261, P)  # fe29.h's Montgomery radix: 9 limbs of 29 bits

_cache: dict = {}
_pow2: dict = {}


def _rng(seed):
    return np.random.default_rng(seed)


def _rand_scalar(rng) -> int:
    return int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1


# ---- points ---------------------------------------------------------------

def _table(Q):
    """2^i Q for i = 0..256 (kept for G and the keys of KEYS)"""
    if Q not in _pow2:
        t = [Q]
        for _ in range(256):
            t.append(p256.point_add(t[-1], t[-1]))
        _pow2[Q] = t
    return _pow2[Q]


def mult(k: int, Q, keep: bool = True):
    """k Q by oracle/p256.py's group law; keep: remember Q's doublings"""
    if not keep and Q not in _pow2:
        return p256.scalar_mult(k, Q)
    t, acc, i = _table(Q), None, 0
    while k:
        if k & 1:
            acc = p256.point_add(acc, t[i])
        k >>= 1
        i += 1
    return acc


def point_at(x: int):
    """the point (x, y) with y = rhs(x)^((p+1)/4), or None"""
    y, ok = wc.sqrt_p(wc.rhs(x))
    return (x, y) if ok else None


def mont_scan(start: int):
    """First point whose Montgomery-form x (x 2^261 mod p) is (start - k) mod p,
    k = 0, 1, ...: (point, k).  k stays below 200, so that a changed constant
    cannot turn the search into a silent skip."""
    inv = pow(R261, -1, P)
    for k in range(200):
        pt = point_at((start - k) % P * inv % P)
        if pt is not None:
            assert pt[0] * R261 % P == (start - k) % P
            return pt, k
    raise AssertionError("no point within 200 of Montgomery x %x" % start)


def keys():
    """KEYS: [(name, (x, y), d or None)] -- d where Q = d G is known."""
    if "keys" in _cache:
        return _cache["keys"]
    rng = _rng(20261)
    out = [("G", G, 1)]
    for i in range(2):  # (their d is thrown away: nothing below uses it)
        out.append(("seeded point %d" % i, mult(_rand_scalar(rng), G), None))
    d64 = int.from_bytes(rng.bytes(8), "big") | (1 << 63)
    for name, d in (("2 G", 2), ("(n - 1) G", N - 1), ("((n + 1) / 2) G", (N + 1) // 2), ("64-bit d G", d64)):
        out.append((name, mult(d, G), d))
    x0 = point_at(0)
    assert x0 is not None and point_at(1 << 32) is not None and point_at(P - 3) is not None
    assert all(point_at(x) is None for x in (1, 2, 3, P - 1, P - 2))
    out.append(("x = 0", x0, None))
    out.append(("x = 0, the other y", (0, P - x0[1]), None))
    out.append(("x = 2^32", point_at(1 << 32), None))
    out.append(("x = p - 3", point_at(P - 3), None))
    # Montgomery-form x with all limbs full, only the top limb short, one top
    # bit, zero, and one full low limb less one
    for what, start, k_want in (("p - 1", P - 1, 0), ("2^232 - 1", (1 << 232) - 1, 0), ("2^255", 1 << 255, 0),
                                ("0", 1, 1), ("2^29 - 2", (1 << 29) - 1, 1)):
        pt, k = mont_scan(start)
        assert k < 200 and k == k_want, (what, k)
        if pt[0] == 0:  # Montgomery form keeps zero: the key "x = 0" above
            assert pt == x0
        else:
            out.append(("Montgomery x = " + what, pt, None))
    assert len(out) == 15 and len({q for _, q, _ in out}) == 15
    assert all(p256.on_curve(q) for _, q, _ in out)
    assert all(d is None or mult(d, G) == q for _, q, d in out)
    _cache["keys"] = out
    return out


def dlog_keys():
    """G and the four d G keys: [(name, Q, d)]"""
    out = [k for k in keys() if k[2] is not None]
    assert len(out) == 5
    return out


# ---- the construction -----------------------------------------------------

def chosen_sig(Q, u1: int, u2: int, variant: str = PLAIN, keep: bool = True):
    """(hash 32 B, r||s 64 B, intended accept bit) of a signature under Q (an
    affine point, or d for Q = d G) whose verify recomputes exactly (u1, u2).
    u1 = 0 is allowed: e = 0.  R at infinity (or r = 0): r = 1, intended 0.
    Variants: FLIP_R (r ^ 2, intended 0: the verifier's u2 changes with it),
    E_PLUS_N (the hash is e + n, which needs e + n < 2^256: in practice e = 0,
    u1 = 0), OTHER_R (s and e are derived from r + 1 instead of r: the verifier
    recomputes the SAME (u1, u2), walks the same points through the same
    meetings, and must reject at the last comparison; intended 0)."""
    if isinstance(Q, int):
        Q = mult(Q, G)
    assert 0 <= u1 < N and 0 < u2 < N
    R = p256.point_add(mult(u1, G), mult(u2, Q, keep))
    r = 0 if R is None else R[0] % N
    want = r != 0
    if r == 0:
        r = 1
    if variant == OTHER_R:
        assert want
        r = r % (N - 1) + 1
        want = False
    s = r * pow(u2, -1, N) % N
    e = u1 * s % N
    if variant == E_PLUS_N:
        e += N
        assert e < 1 << 256
    elif variant == FLIP_R:
        r ^= 2
        want = False
    else:
        assert variant in (PLAIN, OTHER_R)
    return e.to_bytes(32, "big"), r.to_bytes(32, "big") + s.to_bytes(32, "big"), want


class _Rows:
    def __init__(self, family):
        self.family, self.H, self.S, self.K, self.want, self.names, self.rerun = family, [], [], [], [], [], []

    def add(self, name, h, rs, xy: bytes, want, rerun):
        self.H.append(h)
        self.S.append(rs)
        self.K.append(xy)
        self.want.append(bool(want))
        self.names.append(name)
        self.rerun.append(rerun)

    def sig(self, name, key, u1, u2, variant=PLAIN, rerun=None):
        kname, Q, _ = key
        h, rs, want = chosen_sig(Q, u1, u2, variant)
        suffix = "" if variant == PLAIN else " (%s)" % variant
        self.add("%s: %s under %s%s" % (self.family, name, kname, suffix), h, rs, wc.xy_bytes(*Q), want,
                 None if variant == FLIP_R else rerun)  # (a flipped r changes u2; the other variants keep both scalars)
        return want

    def done(self, oracle_lib):
        n = len(self.H)
        H = np.frombuffer(b"".join(self.H), np.uint8).reshape(n, 32).copy()
        S = np.frombuffer(b"".join(self.S), np.uint8).reshape(n, 64).copy()
        K = np.frombuffer(b"".join(self.K), np.uint8).reshape(n, 64).copy()
        want = np.array(self.want, bool)
        got = np.zeros(n, bool)
        for i in range(n):
            got[i] = oracle_lib.oracle_ecdsa_p256_verify(H[i].ctypes.data, S[i].ctypes.data, K[i].ctypes.data) == 1
        bad = [self.names[i] for i in np.nonzero(got != want)[0]]
        assert not bad, bad[:4]
        assert want.any() and not want.all(), self.family  # every family holds accepted and rejected cases
        return H, S, K, want, list(self.names), list(self.rerun), [self.family] * n


# ---- ladder ---------------------------------------------------------------

def ladder_scalars():
    """[(name, u2)], each 0 < u2 < n, no value twice"""
    out, seen = [], set()

    def put(name, u):
        if 0 < u < N and u not in seen:
            seen.add(u)
            out.append((name, u))

    for k in range(64):
        for v in range(1, 16):
            if k in (0, 1, 31, 62, 63) or v in (1, 7, 8, 9, 15):
                put("u2 = %x * 16^%d" % (v, k), v << (4 * k))
    for nib in (8, 9, 15):
        for start in (0, 32):
            for length in range(1, 65 - start):
                put("u2 = %d nibbles %X from nibble %d" % (length, nib, start),
                    int("%X" % nib * length, 16) << (4 * start))
    put("u2 = 88..88", int("8" * 64, 16))
    put("u2 = 88..89", int("8" * 63 + "9", 16))
    # The sets above leave the digits +-2 .. +-6 (-6 excepted: the runs of 9)
    # open at most positions: 16 scalars whose digit at position i is
    # ((i + rot) mod 16) - 7 for i < 63, under a top digit 1, close that.
    for rot in range(16):
        u = (1 << 252) + sum((((i + rot) % 16) - 7) << (4 * i) for i in range(63))
        put("u2 = digits rotated by %d" % rot, u)
    return out


def _ladder_coverage(scalars):
    pairs, first, top = set(), set(), False
    for u in scalars:
        d = [x for x, _ in signed_digits(u, [4] * 65)]
        assert sum(x << (4 * i) for i, x in enumerate(d)) == u and all(-7 <= x <= 8 for x in d)
        pairs.update((i, x) for i, x in enumerate(d[:64]))
        first.add(max(i for i, x in enumerate(d) if x != 0))
        top = top or d[64] == 1
    missing = [(i, x) for i in range(64) for x in range(-7, 9) if (i, x) not in pairs]
    assert not missing, missing[:8]
    assert top, "no scalar with d_64 = 1"
    assert first >= set(range(65)), sorted(set(range(65)) - first)  # the infinity start at every position


def ladder(oracle_lib):
    if "ladder" in _cache:
        return _cache["ladder"]
    K, rows = keys(), _Rows("ladder")
    u1_fixed = _rand_scalar(_rng(20262))
    scalars = ladder_scalars()
    digits8 = [x for x, _ in signed_digits(int("8" * 64, 16), [4] * 65)]
    digits9 = [x for x, _ in signed_digits(int("8" * 63 + "9", 16), [4] * 65)]
    assert digits8[64] == 0 and digits9[64] == 1  # the boundary pair of the carry chain
    j = 0
    for name, u2 in scalars:
        for t in (0, 5, 11):  # three keys, G only where the rotation lands on it
            key = K[(j + t) % len(K)]
            u1 = 0 if j % 2 == 0 else u1_fixed
            variant = PLAIN
            if j % 8 == 2:
                variant = E_PLUS_N  # (u1 = 0: the hash is n itself)
            elif j % 8 == 5:
                variant = FLIP_R
            rows.sig(name, key, u1, u2, variant, rerun=False)
            j += 1
    for k in (1, 2, 3):
        for i, key in enumerate(K):
            # u2 = n - 2: the ladder's LAST addition is -Q + -Q whatever Q is (varbase.h)
            rows.sig("u2 = n - %d" % k, key, 0 if i % 2 else u1_fixed, N - k, rerun=k == 2)
    _ladder_coverage([u for _, u in scalars] + [N - 1, N - 2, N - 3])
    assert sum(1 for r in rows.rerun if r) == len(K)
    _cache["ladder"] = rows.done(oracle_lib)
    return _cache["ladder"]


# ---- G part ---------------------------------------------------------------

def gdigits(u1: int) -> list:
    d = [x for x, _ in signed_digits(u1, [16] * 17)]
    assert sum(x << (16 * i) for i, x in enumerate(d)) == u1
    return d


def u1_from_gdigits(d) -> int:
    """the scalar whose 17 comb digits are d (the recoding is unique)"""
    u = sum(x << (16 * i) for i, x in enumerate(d))
    assert 0 < u < N and gdigits(u) == list(d), d
    return u


def meeting_u2(u1: int, window: int, d: int, cancel: bool) -> int:
    """u2 under Q = d G such that the accumulator before G window `window`,
    (u2 d + sum_{j < window} g_j 2^(16 j)) G, equals the window's own point
    g_i 2^(16 i) G (the unchecked addition is then a doubling) or its negative
    (a cancellation: the sum is at infinity after this window)."""
    g = gdigits(u1)
    assert g[window] != 0
    before = sum(g[j] << (16 * j) for j in range(window))
    target = (-1 if cancel else 1) * (g[window] << (16 * window))
    u2 = (target - before) * pow(d, -1, N) % N
    assert 0 < u2 < N and (u2 * d + before - target) % N == 0
    return u2


def gpart(oracle_lib):
    if "gpart" in _cache:
        return _cache["gpart"]
    rng, rows, DK = _rng(20263), _Rows("gpart"), dlog_keys()
    u1s = []

    def rand_digit():
        return int(rng.integers(1, 32767)) * (1 if rng.integers(0, 2) else -1)

    # plain: the digit g at window w among seeded nonzero digits; nothing meets
    j = 0
    for w in range(16):
        for g in (1, -1, 2, 32767, 32768, -32767):
            d = [rand_digit() for _ in range(16)] + [0]
            d[15] = abs(d[15])
            d[w] = g
            d[16] = 1 if d[15] < 0 else 0
            u1 = u1_from_gdigits(d)
            assert gdigits(u1)[w] == g
            u1s.append(u1)
            for t in (0, 2):
                rows.sig("digit %d at G window %d" % (g, w), DK[(j + t) % 5], u1, _rand_scalar(rng), rerun=False)
            j += 1
    # the 17th window is only ever the carry: g_16 = 1 over g_15 = -1 and over g_15 = 0
    for top, g15 in ((0xFFFF8000 << 224, -1), (0xFFFF8001 << 224, 0)):
        u1 = top + int.from_bytes(rng.bytes(27), "big")
        assert u1 < N and gdigits(u1)[16] == 1 and gdigits(u1)[15] == g15
        u1s.append(u1)
        for key in DK:
            rows.sig("g_16 = 1 over g_15 = %d" % g15, key, u1, _rand_scalar(rng), rerun=False)
    # meetings: a doubling and a cancellation at windows 0, 1, 15 and 16, and a
    # cancellation at window 7 that the sum continues from; placed last, next
    # to the SEC1 family's rejected keys in combined()'s natural order
    u1_low = u1_from_gdigits([rand_digit() for _ in range(15)] + [int(rng.integers(1, 32767)), 0])
    u1_top = (0xFFFF8001 << 224) + int.from_bytes(rng.bytes(27), "big")
    assert u1_top >= 0xFFFF8001 << 224 and u1_top < N and gdigits(u1_top)[16] == 1
    u1s += [u1_low, u1_top]
    accepted = 0

    def meeting(name, key, u1, u2):
        # ... and where R is finite, its twin with another r over the same
        # scalars: a Z == 0 result taken for a finite point compares 0 == r * 0
        nonlocal accepted
        if rows.sig(name, key, u1, u2, rerun=True):
            accepted += 1
            rows.sig(name, key, u1, u2, OTHER_R, rerun=True)

    for key in DK:
        for w in (0, 1, 15, 16):
            u1 = u1_top if w == 16 else u1_low
            for cancel in (False, True):
                what = "cancellation" if cancel else "doubling"
                meeting("%s at G window %d" % (what, w), key, u1, meeting_u2(u1, w, key[2], cancel))
        assert any(gdigits(u1_low)[8:])
        meeting("cancellation at G window 7, the sum continues", key, u1_low, meeting_u2(u1_low, 7, key[2], True))
    assert accepted == 5 * 7  # (a cancellation at the last nonzero window ends at infinity: rejected)
    _cache["gpart_u1"] = u1s
    _cache["gpart"] = rows.done(oracle_lib)
    return _cache["gpart"]


# ---- key shape ------------------------------------------------------------

def gpart_u1s(oracle_lib) -> list:
    """every u1 of the G-part family, for a digit-by-digit check of vb_next_gdigit"""
    gpart(oracle_lib)
    return _cache["gpart_u1"]


def keyshape(oracle_lib):
    if "keyshape" in _cache:
        return _cache["keyshape"]
    rng, rows = _rng(20264), _Rows("keyshape")
    for key in keys():
        for i in range(4):
            u1, u2 = _rand_scalar(rng), _rand_scalar(rng)
            rows.sig("seeded scalars %d" % i, key, u1, u2, rerun=False)
            rows.sig("seeded scalars %d" % i, key, u1, u2, FLIP_R)
    _cache["keyshape"] = rows.done(oracle_lib)
    return _cache["keyshape"]


# ---- SEC1 -----------------------------------------------------------------

def sec1_xs(n_random: int = 512):
    xs = list(range(256)) + list(range(P - 256, P)) + list(range(P, P + 4))
    for k in range(8, 256, 8):
        xs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    rng = _rng(20265)
    xs += [int.from_bytes(rng.bytes(32), "big") for _ in range(n_random)]
    assert sum(1 for x in range(2000) if point_at(x) is not None) == 1003
    return xs


def sec1(oracle_lib):
    """Every X under 02 and under 03.  An X with a point carries a signature
    with seeded full-length scalars under the key the prefix decodes to
    (accepted); an X without one, or >= p, carries its predecessor's signature
    (rejected).  Returns the usual columns; sec1_compressed() gives the keys."""
    if "sec1" in _cache:
        return _cache["sec1"]
    rng, rows = _rng(20266), _Rows("sec1")
    xs = sec1_xs()
    have = 0
    prev = None
    for x in xs:
        for prefix in (2, 3):
            comp = bytes([prefix]) + x.to_bytes(32, "big")
            pt = wc.decode(comp, wc.KEY_COMPRESSED)
            if pt is not None:
                have += 1
                assert p256.on_curve(pt) and pt[0] == x and (pt[1] & 1) == (prefix & 1)
                h, rs, want = chosen_sig(pt, _rand_scalar(rng), _rand_scalar(rng), keep=False)
                assert want
                prev = (h, rs)
                rows.add("sec1: X = %x under %02x" % (x, prefix), h, rs, wc.xy_bytes(*pt), True, False)
            else:
                assert prev is not None
                assert x >= P or wc.rhs(x) not in (0, 1)  # X || parity is then off the curve as X||Y too
                rows.add("sec1: X = %x under %02x, no point" % (x, prefix), prev[0], prev[1],
                         x.to_bytes(32, "big") + (prefix & 1).to_bytes(32, "big"), False, None)
    assert 0.4 * 2 * len(xs) <= have <= 0.6 * 2 * len(xs), (have, len(xs))
    out = rows.done(oracle_lib)
    comp = wc.encode(out[2], wc.KEY_COMPRESSED)
    want = [bytes([pre]) + x.to_bytes(32, "big") for x in xs for pre in (2, 3)]
    assert [c.tobytes() for c in comp] == want  # the rows encode to exactly the swept keys
    _cache["sec1"] = out
    return out


# ---- all of it ------------------------------------------------------------

def family(oracle_lib, name):
    return {"ladder": ladder, "gpart": gpart, "keyshape": keyshape, "sec1": sec1}[name](oracle_lib)


def kinds(want_key_ok, rerun) -> np.ndarray:
    k = np.full(len(rerun), KIND_PLAIN, np.int8)
    k[[i for i, r in enumerate(rerun) if r]] = KIND_RERUN
    k[~np.asarray(want_key_ok, bool)] = KIND_REJECTED_KEY
    return k


def _some_wave_holds_all_kinds(kind) -> bool:
    return any(set(kind[i:i + 64].tolist()) >= {KIND_PLAIN, KIND_RERUN, KIND_REJECTED_KEY}
               for i in range(0, len(kind), 64))


def combined(oracle_lib):
    """All families: a dict with hashes, sigs, xy, want (under X||Y), names,
    rerun, family, key_ok (X||Y is a point), and perm -- one seeded permutation
    of the rows.  In the natural order (ladder, key shape, G part, SEC1) and
    under perm some 64-aligned window holds a rerun lane, a rejected key and a
    plain lane side by side."""
    if "combined" in _cache:
        return _cache["combined"]
    parts = [family(oracle_lib, f) for f in ("ladder", "keyshape", "gpart", "sec1")]
    H, S, K, want = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    names, rerun, fam = (sum((p[i] for p in parts), []) for i in (4, 5, 6))
    key_ok = np.array([wc.decode(k.tobytes(), wc.KEY_XY) is not None for k in K], bool)
    assert not want[~key_ok].any()
    kind = kinds(key_ok, rerun)
    perm = _rng(20267).permutation(len(H))
    assert _some_wave_holds_all_kinds(kind), "natural order: no wave with all three kinds"
    assert _some_wave_holds_all_kinds(kind[perm]), "permuted order: no wave with all three kinds"
    assert 2000 <= len(H) <= 9000
    _cache["combined"] = dict(hashes=H, sigs=S, xy=K, want=want, names=names, rerun=rerun, family=fam, key_ok=key_ok,
                              kind=kind, perm=perm)
    return _cache["combined"]


def ordered(c, order: str):
    """(hashes, sigs, xy, want, index) of combined() in 'natural' or 'permuted' order"""
    idx = np.arange(len(c["want"])) if order == "natural" else c["perm"]
    assert order in ("natural", "permuted")
    return tuple(np.ascontiguousarray(c[k][idx]) for k in ("hashes", "sigs", "xy", "want")) + (idx,)


def wire(oracle_lib, hashes, sigs, xy, fmt):
    """(keys in fmt, expected bits): the oracle's verdict under Python's decode
    of the encoded key (wirekey_cases.expect), 0 where Python rejects it"""
    k = wc.encode(xy, fmt)
    return k, wc.expect(oracle_lib, hashes, sigs, k, fmt)
