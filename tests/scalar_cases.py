"""Chosen-s signatures for every on-device inversion mod n, shared by
tests/test_scalar_cases.py (CPU) and tests/test_gpu_scalar_seams.py (GPU).

The hash is a free input of the batch verify, so a VALID signature exists for
any chosen s; a wrong s^-1 on the device then turns an expected 1 into a 0.

  fixed key, chosen s   key d, one nonce k, r = x(k G) mod n; for any s in
                        (0, n) the hash is e = (s k - r d) mod n.  One scalar
                        multiplication serves every signature.
  free key, chosen      lift x_R to a point R, r = x_R mod n, e any 256-bit
  (x_R, s, e)           value, u1 = e / s, Q = (s / r) (R - u1 G): Q is that
                        signature's key.
  twin                  the same hash and s, r replaced by r xor 2: rejected
                        (asserted with the oracle).  Never made by changing s:
                        s xor 1 of (n + 1) / 2 is -s, the valid high-S form.

S_EDGE (s_edge()) is the list of chosen s; GRID (grid()) the free-key triples;
GROUPS (groups(K)) are batches for the lane path (k_ecdsa_scalars<K>) in which
the value that a wave's or a block's SHARED inversion receives, (prod s) 2^261
mod n over the group's in-range s, is a chosen target.

Known limit of groups(): the membership rule (ownership()) restates the
comment above k_ecdsa_scalars and launch_scalars_k -- L = 256 ceil(ceil(n / K)
/ 256) lanes, lane l owns signatures l + j L, the group is the wave for K <= 2
and the block for K >= 4.  If it drifts from the kernel, the totals become
random values and the GPU test still passes: it then tests no less than a
random batch, but no longer what it claims.

Everything is seeded; expected bits come from the oracle, and the module also
says which signatures are valid by construction so that the agreement cannot be
vacuous."""
from __future__ import annotations

import random
from functools import lru_cache

import numpy as np

import safegcd_model as model
from oracle import p256

N, P = p256.N, p256.P
M30 = (1 << 30) - 1
R261 = (1 << 261) % N
OUT_OF_RANGE = (0, N, (1 << 256) - 1)
N_KEYS = 12
N_RANDOM_SEARCH = 20000


def _rng(tag: str) -> random.Random:
    return random.Random("scalar_cases/" + tag)


def _b32(v: int) -> bytes:
    return v.to_bytes(32, "big")


# ---- curve arithmetic for the constructions (Jacobian, a = -3) --------------
def _jdbl(X, Y, Z):
    if Y == 0 or Z == 0:
        return 0, 1, 0
    d, g = Z * Z % P, Y * Y % P
    b = X * g % P
    a = 3 * (X - d) * (X + d) % P
    X3 = (a * a - 8 * b) % P
    return X3, (a * (4 * b - X3) - 8 * g * g) % P, 2 * Y * Z % P


def _jadd_affine(X1, Y1, Z1, x2, y2):
    if Z1 == 0:
        return x2, y2, 1
    zz = Z1 * Z1 % P
    h, r = (x2 * zz - X1) % P, (y2 * Z1 * zz - Y1) % P
    if h == 0:
        return _jdbl(X1, Y1, Z1) if r == 0 else (0, 1, 0)
    h2 = h * h % P
    h3, v = h * h2 % P, X1 * h2 % P
    X3 = (r * r - h3 - 2 * v) % P
    return X3, (r * (v - X3) - Y1 * h3) % P, Z1 * h % P


def smul(k: int, pt):
    """k * pt (affine or None), left to right; checked against p256.scalar_mult
    in tests/test_scalar_cases.py."""
    k %= N
    if pt is None or k == 0:
        return None
    X, Y, Z = 0, 1, 0
    for bit in bin(k)[2:]:
        X, Y, Z = _jdbl(X, Y, Z)
        if bit == "1":
            X, Y, Z = _jadd_affine(X, Y, Z, pt[0], pt[1])
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def lift_x(x: int):
    """(x, y) on the curve with the root y = rhs^((p+1)/4), or None."""
    rhs = (x * x * x - 3 * x + p256.B) % P
    y = pow(rhs, (P + 1) // 4, P)
    return (x, y) if y * y % P == rhs else None


def usable_x(x: int) -> bool:
    """x is the abscissa of a point, and r = x mod n and r xor 2 (the twin's) lie inside (0, n)"""
    return lift_x(x) is not None and 0 < x % N and 0 < (x % N) ^ 2 < N


def curve_x_from(x: int, step: int) -> int:
    """the first usable x' = x, x + step, x + 2 step, .."""
    while not usable_x(x):
        x += step
    return x


# ---- S_EDGE -----------------------------------------------------------------
def _limb_patterns(rng):
    out = []
    seams = (("2^29-1", (1 << 29) - 1), ("2^29", 1 << 29), ("2^29+1", (1 << 29) + 1), ("2^30-1", M30))
    for name, v in seams:
        for j in range(8):
            while True:
                x = (rng.randrange(1 << 256) & ~(M30 << (30 * j))) | (v << (30 * j))
                if 0 < x < N:
                    break
            out.append(("limb30", "limb %d = %s" % (j, name), x))
    for name, v in seams:
        while True:
            x = sum(v << (30 * j) for j in range(8)) | (rng.randrange(1 << 16) << 240)
            if x < N:
                break
        out.append(("limb30-all", "all limbs = %s" % name, x))
    out.append(("limb30-low", "low 30 bits zero", rng.randrange(1 << 30, N) & ~M30))
    out.append(("limb30-low", "low 60 bits zero", rng.randrange(1 << 60, N) & ~((1 << 60) - 1)))
    for j in range(8):
        for w in (0, 0xFFFFFFFF):
            while True:
                x = (rng.randrange(1 << 256) & ~(0xFFFFFFFF << (32 * j))) | (w << (32 * j))
                if j == 7 and w:  # below n only with word 6 = 0
                    x &= ~(0xFFFFFFFF << 192)
                if 0 < x < N:
                    break
            out.append(("word32", "word %d = %08x" % (j, w), x))
    out.append(("limb29", "all nine 29-bit limbs = 2^29-1 (mod n)", (1 << 261) - 1))
    out.append(("limb29", "low eight 29-bit limbs = 2^29-1", ((1 << 232) - 1) | (rng.randrange(1 << 23) << 232)))
    return out


@lru_cache(maxsize=None)
def _base_edges():
    raw = [("small", str(v), v) for v in (1, 2, 3)]
    raw += [("small", "n-%d" % v, N - v) for v in (1, 2, 3)]
    raw += [("half", "(n-1)/2", (N - 1) // 2), ("half", "(n+1)/2", (N + 1) // 2)]
    raw += [("2^k", "2^%d" % k, 1 << k) for k in range(256)]
    raw += [("2^k-1", "2^%d-1" % k, (1 << k) - 1) for k in range(2, 256)]
    raw += [("2^k+1", "2^%d+1" % k, (1 << k) + 1) for k in range(1, 256)]
    raw += [("n-2^k", "n-2^%d" % k, N - (1 << k)) for k in range(256)]
    raw += _limb_patterns(_rng("limbs"))
    return tuple(raw)


@lru_cache(maxsize=None)
def model_search():
    """safegcd_model.inv_stats over the chosen values and N_RANDOM_SEARCH
    seeded random ones: {"stats": {x: (batches, max_eta, max_d)}, "random":
    [x, ..], "picks": [(class, label, x), ..]}."""
    rng = _rng("search")
    rnd = [rng.randrange(1, N) for _ in range(N_RANDOM_SEARCH)]
    pool = sorted({v % N for _, _, v in _base_edges()} - {0}) + rnd
    stats = {}
    for x in pool:
        if x not in stats:
            D, b, me, md = model.inv_stats(x)
            assert D % N == R261 * pow(x, -1, N) % N
            stats[x] = (b, me, md)
    xs = sorted(stats)
    picks = [("model", "fewest batches (%d)" % stats[x][0], x) for x in sorted(xs, key=lambda x: (stats[x][0], x))[:4]]
    picks += [("model", "most batches (%d)" % stats[x][0], x) for x in sorted(xs, key=lambda x: (-stats[x][0], x))[:4]]
    x = max(xs, key=lambda x: (stats[x][1], x))
    picks.append(("model", "largest |eta| (%d)" % stats[x][1], x))
    x = max(xs, key=lambda x: (stats[x][2], x))
    picks.append(("model", "largest |d|/n (%.3f)" % stats[x][2], x))
    return {"stats": stats, "random": rnd, "picks": picks}


@lru_cache(maxsize=None)
def s_edge():
    """[(class, label, s)]: every s in (0, n), no duplicates (the first label stays)."""
    rng = _rng("random-s")
    raw = list(_base_edges()) + model_search()["picks"]
    raw += [("random", "random %d" % i, rng.randrange(1, N)) for i in range(64)]
    seen, out = set(), []
    for cls, label, v in raw:
        v %= N
        if v and v not in seen:
            seen.add(v)
            out.append((cls, label, v))
    return tuple(out)


def edge_value(label: str) -> int:
    return next(v for _, l, v in s_edge() if l == label)


# ---- fixed keys, chosen s ------------------------------------------------------
@lru_cache(maxsize=None)
def fixed_keys():
    """(private keys, keys (N_KEYS, 64) uint8, nonce k, r = x(k G) mod n)"""
    rng = _rng("keys")
    ds = [rng.randrange(1, N) for _ in range(N_KEYS)]
    keys = np.zeros((N_KEYS, 64), np.uint8)
    for i, d in enumerate(ds):
        q = smul(d, p256.G)
        keys[i] = np.frombuffer(_b32(q[0]) + _b32(q[1]), np.uint8)
    while True:
        k = rng.randrange(1, N)
        r = smul(k, p256.G)[0] % N
        if 0 < r ^ 2 < N and r:  # (the twin stays inside Go's range checks)
            return ds, keys, k, r


def fixed_hash(s: int, key: int = 0) -> int:
    ds, _, k, r = fixed_keys()
    return (s * k - r * ds[key]) % N


def _arrays(rows):
    """[(hash int, r int, s int)] -> hashes (n, 32), sigs (n, 64) uint8"""
    hb = b"".join(_b32(e) for e, _, _ in rows)
    sb = b"".join(_b32(r) + _b32(s) for _, r, s in rows)
    n = len(rows)
    return (np.frombuffer(hb, np.uint8).reshape(n, 32).copy(), np.frombuffer(sb, np.uint8).reshape(n, 64).copy())


@lru_cache(maxsize=None)
def edge_signatures():
    """Every S_EDGE value as a signature under fixed key 0, each followed by
    its twin: {"hashes", "sigs", "kidx", "valid", "labels", "s"}."""
    _, _, _, r = fixed_keys()
    rows, valid, labels, ss = [], [], [], []
    for _, label, s in s_edge():
        e = fixed_hash(s)
        rows += [(e, r, s), (e, r ^ 2, s)]
        valid += [True, False]
        labels += [label, label + " (twin)"]
        ss += [s, s]
    h, sg = _arrays(rows)
    return {"hashes": h, "sigs": sg, "kidx": np.zeros(len(rows), np.uint32), "valid": np.array(valid, bool),
            "labels": labels, "s": ss}


# ---- GRID: free key, chosen (x_R, s, e) -----------------------------------------
@lru_cache(maxsize=None)
def grid_components():
    rng = _rng("grid")
    es = [("0", 0), ("1", 1), ("n-1", N - 1), ("n", N), ("n+1", N + 1), ("2^255", 1 << 255), ("2^256-1", (1 << 256) - 1),
          ("random < n", rng.randrange(1, N)), ("random >= n", rng.randrange(N, 1 << 256))]
    xs = [("smallest x", curve_x_from(0, 1)),
          ("largest x < p-n", curve_x_from(P - N - 1, -1)),
          ("smallest x >= p-n", curve_x_from(P - N, 1)),
          ("largest x < n", curve_x_from(N - 1, -1)),
          ("smallest x in [n, p)", curve_x_from(N, 1)),
          ("largest x < p", curve_x_from(P - 1, -1))]
    ss = [("1", 1), ("n-1", N - 1), ("(n+1)/2", (N + 1) // 2), ("2^255", 1 << 255),
          ("random a", rng.randrange(1, N)), ("random b", rng.randrange(1, N))]
    return es, xs, ss


def free_key_signature(x_r: int, s: int, e: int):
    """(r, key (x, y)): the signature (r, s) of the 256-bit hash value e is
    valid under the key, and the verifier's sum is the lift of x_r."""
    Rp = lift_x(x_r)
    r = x_r % N
    assert Rp is not None and r != 0
    u1 = e * pow(s, -1, N) % N
    g = smul(u1, p256.G)
    diff = p256.point_add(Rp, None if g is None else (g[0], (P - g[1]) % P))
    q = smul(s * pow(r, -1, N) % N, diff)
    assert q is not None
    return r, q


@lru_cache(maxsize=None)
def grid():
    """The 9 x 6 x 6 = 324 triples, each followed by its twin: {"hashes",
    "sigs", "pubs" (n, 64), "valid", "labels"}."""
    es, xs, ss = grid_components()
    rows, pubs, valid, labels = [], [], [], []
    for en, e in es:
        for xn, x in xs:
            for sn, s in ss:
                r, q = free_key_signature(x, s, e)
                assert 0 < r ^ 2 < N
                rows += [(e, r, s), (e, r ^ 2, s)]
                pubs += [_b32(q[0]) + _b32(q[1])] * 2
                valid += [True, False]
                label = "e=%s x_R=%s s=%s" % (en, xn, sn)
                labels += [label, label + " (twin)"]
    h, sg = _arrays(rows)
    return {"hashes": h, "sigs": sg, "pubs": np.frombuffer(b"".join(pubs), np.uint8).reshape(len(rows), 64).copy(),
            "valid": np.array(valid, bool), "labels": labels}


def grid_registered():
    """grid() with its distinct keys as a table: (keys (324, 64), kidx)."""
    g = grid()
    return np.ascontiguousarray(g["pubs"][0::2]), (np.arange(len(g["valid"])) // 2).astype(np.uint32)


# ---- GROUPS: chosen totals for the lane path's shared inversions --------------------
def ownership(K: int, n: int):
    """(L, lane, j, group) of every signature index (the rule restated from
    k_ecdsa_scalars / launch_scalars_k, see the module docstring)."""
    lanes = -(-n // K)
    L = 256 * -(-lanes // 256)
    i = np.arange(n, dtype=np.int64)
    lane = i % L
    return L, lane, i // L, lane // (64 if K <= 2 else 256)


def required_targets():
    picks = model_search()["picks"]
    out = [("1", 1), ("2", 2), ("n-1", N - 1), ("2^255", 1 << 255), ("2^30", 1 << 30)]
    out += [(l, edge_value(l)) for l in ("all limbs = 2^29-1", "all limbs = 2^29", "all limbs = 2^29+1",
                                         "all limbs = 2^30-1", "low 30 bits zero", "low 60 bits zero")]
    out += [(picks[0][1], picks[0][2]), (picks[4][1], picks[4][2])]
    return out


SPECIALS = ("1", "2", "n-1", "2^255", "2^30", "(n+1)/2", "all limbs = 2^29", "all limbs = 2^30-1", "2^29-1", "n-2^29",
            "2^255+1", "word 0 = ffffffff")
SPECIAL_LANES = (0, 63, 64, 255)


def group_total(svals) -> int:
    """what the shared inversion receives: (prod of the in-range s) 2^261 mod n"""
    t = R261
    for s in svals:
        if 0 < s < N:
            t = t * s % N
    return t


@lru_cache(maxsize=None)
def groups(K: int):
    """One batch for k_ecdsa_scalars<K>: {"K", "n", "L", "hashes", "sigs",
    "kidx", "valid" (valid by construction), "kind" (per signature: "valid",
    "twin", "out", "r=0", "r=n", "key"), "s" (ints), "groups": [{"kind":
    "target" | "ones" | "out", "target", "members", "solved"}], "special":
    {(j, lane in block): label}} under the N_KEYS fixed keys (key of
    signature i: i mod N_KEYS).

    28 waves for K <= 2 and 15 blocks for K >= 4 -- the 13 targets of
    required_targets() (more from S_EDGE where there is room), one group of
    s = 1 throughout and one with every s out of range -- and 13 signatures
    short of full, so the last lanes own one signature fewer: n = 1779, 3571,
    15 347, 30 707, 61 427 for K = 1, 2, 4, 8, 16."""
    assert K in (1, 2, 4, 8, 16)
    rng = _rng("groups %d" % K)
    width = 64 if K <= 2 else 256
    ng = 28 if K <= 2 else 15
    Lw = ng * width
    n = K * Lw - 13  # not a multiple of 256 K: the last lanes own one signature fewer (K = 1: none)
    L, lane, jj, grp = ownership(K, n)
    assert L == Lw and int(grp.max()) == ng - 1
    ds, _, k, r = fixed_keys()
    g_ones, g_out = (5, 18) if K <= 2 else (3, 8)
    targets = required_targets()
    pool = [x for x in s_edge() if x[0] != "random"]
    while len(targets) < ng - 2:
        _, label, v = pool[rng.randrange(len(pool))]
        if all(v != t for _, t in targets):
            targets.append((label, v))
    members = [np.nonzero(grp == g)[0] for g in range(ng)]
    ginfo, titer = [], iter(targets)
    for g in range(ng):
        kind = "ones" if g == g_ones else "out" if g == g_out else "target"
        label, t = next(titer) if kind == "target" else ("2^261 mod n", R261)
        ginfo.append({"kind": kind, "target": t, "label": label, "members": members[g], "solved": None})
    # the last group (ragged) is a targeted one
    assert ginfo[-1]["kind"] == "target" and len(members[-1]) < K * width
    s = [None] * n
    kind = ["valid"] * n
    for i in members[g_ones]:
        s[i] = 1
    for c, i in enumerate(members[g_out]):
        s[i], kind[i] = OUT_OF_RANGE[c % 3], "out"
    # a special s at every j and at lanes 0, 63, 64, 255 of a block of targeted groups
    nblocks = L // 256
    blocks_ok = [b for b in range(nblocks)
                 if all(ginfo[int(g)]["kind"] == "target" for g in set(grp[(lane // 256 == b)].tolist()))]
    special, c = {}, 0
    for j in range(K):
        b = blocks_ok[j % len(blocks_ok)]
        for ln in SPECIAL_LANES:
            i = b * 256 + ln + j * L
            assert i < n and s[i] is None
            s[i] = edge_value(SPECIALS[c % len(SPECIALS)])
            special[(j, ln)] = SPECIALS[c % len(SPECIALS)]
            c += 1
    tg = [g for g in range(ng) if ginfo[g]["kind"] == "target"]
    for g in tg:  # the last free member is the solved one
        ginfo[g]["solved"] = int(max(i for i in members[g] if s[i] is None))
        s[ginfo[g]["solved"]] = 0  # (placeholder: solved below)
    # out-of-range members beside in-range ones (they join as 1) in four targeted groups
    for g in (tg[0], tg[1], tg[2], tg[-1]):
        free = [int(i) for i in members[g] if s[i] is None]
        for c, i in enumerate(rng.sample(free, 6)):
            s[i], kind[i] = OUT_OF_RANGE[c % 3], "out"
    # members rejected for another reason: their in-range s stays in the product
    for g in (tg[1], tg[3], tg[-1]):
        free = [int(i) for i in members[g] if s[i] is None]
        for what, i in zip(("r=0", "r=n", "key"), rng.sample(free, 3)):
            s[i], kind[i] = rng.randrange(1, N), what
    # every S_EDGE value somewhere, then random ones (some as twins)
    free = [i for i in range(n) if s[i] is None]
    rng.shuffle(free)
    edges = [v for _, _, v in s_edge()]
    assert len(free) >= len(edges)
    for c, i in enumerate(free):
        if c < len(edges):
            s[i] = edges[c]
        else:
            s[i] = rng.randrange(1, N)
            if rng.random() < 0.03:
                kind[i] = "twin"
    for g in tg:
        i = ginfo[g]["solved"]
        others = group_total(s[m] for m in members[g] if m != i)
        s[i] = ginfo[g]["target"] * pow(others, -1, N) % N
        assert 0 < s[i] < N
    rows, kidx = [], np.zeros(n, np.uint32)
    for i in range(n):
        key = i % N_KEYS
        kidx[i] = key
        si, kd = s[i], kind[i]
        e = rng.randrange(1 << 256) if kd == "out" else (si * k - r * ds[key]) % N
        rr = {"valid": r, "out": r, "twin": r ^ 2, "r=0": 0, "r=n": N, "key": r}[kd]
        if kd == "key":
            kidx[i] = N_KEYS + i % 5
        rows.append((e, rr, si))
    h, sg = _arrays(rows)
    return {"K": K, "n": n, "L": L, "hashes": h, "sigs": sg, "kidx": kidx,
            "valid": np.array([kd == "valid" for kd in kind], bool), "kind": kind, "s": s, "groups": ginfo,
            "special": special}


# ---- expected bits -----------------------------------------------------------------
def oracle_keyed(oracle_lib, hashes, sigs, keys, kidx) -> np.ndarray:
    """oracle_ecdsa_p256_verify_batch over a key table (a key index past it: 0)."""
    n = len(kidx)
    hashes, sigs = np.ascontiguousarray(hashes, np.uint8), np.ascontiguousarray(sigs, np.uint8)
    keys, kidx = np.ascontiguousarray(keys, np.uint8), np.ascontiguousarray(kidx, np.uint32)
    bm = np.zeros((n + 7) // 8, np.uint8)
    oracle_lib.oracle_ecdsa_p256_verify_batch(hashes.ctypes.data, sigs.ctypes.data, kidx.ctypes.data, n,
                                              keys.ctypes.data, len(keys), bm.ctypes.data, 8)
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


def oracle_own_key(oracle_lib, hashes, sigs, pubs) -> np.ndarray:
    """the same for signature i under pubs[i]"""
    return oracle_keyed(oracle_lib, hashes, sigs, pubs, np.arange(len(pubs), dtype=np.uint32))
