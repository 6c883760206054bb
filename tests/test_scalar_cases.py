"""The chosen-s cases of tests/scalar_cases.py and the inversion model of
tests/safegcd_model.py, checked on the CPU: the lists hold what they claim,
every inverse is right under the portable safegcd (h_inv_n_words, _ct) and the
lane-limb model, every crafted signature is valid under both oracles and every
twin and broken member rejected, the CPU build of the scalar stage (h_scalars)
returns e / s and r / s, and the groups' totals are their targets.

Measured with the seeds of scalar_cases.py (21 079 distinct inputs: the 1 079
chosen values before the model's picks and 20 000 random ones):

  batches per inversion   16: 7    17: 197    18: 18 598    19: 2 277
  random inputs alone     17: 72   18: 17 684  19: 2 244
  minimum 16 (2^k for k = 124 .. 127 and 158 .. 160, nothing else),
  maximum 19; largest |eta| between batches 241 (s = 2^255); largest |d| / n
  0.832 (the kernel's fix-up + 16 n allows 13.5).

So the first 14 untested batches of inv_mod_n_wave never see g = 0 on any
input found, and its "g == 0 in an untested batch" path has no known input.

Event coverage of divsteps30_scalar's control flow over S_EDGE (state of the
STEP x what follows it), all of it reached:

            fast-swap  rare-swap  rare-elim  exit
     S0        yes        yes        yes      yes
     S1        yes      (never)      yes      yes
     S2        yes      (never)      yes      yes
     S3        yes      (never)      yes      yes

The rare path's swap in S1..S3 cannot be reached by any input: the fast test
"old e1 <= z" (unsigned) misses a swap only when e1 is negative at the STEP,
e1 is >= 1 after every swap (2 - e1', e1' <= 0) and every elimination, so it
is negative only at a batch's first STEP, which is always made in S0.
divsteps30_states asserts that invariant on every STEP; the three branches
are dead code in the kernel, harmless.  Elimination widths: 1..6 limited by
e1, 1..6 limited by i, 6 by the cap -- all reached; the cap is the constant 6,
so it limits no other width."""
from __future__ import annotations

import ctypes
import random
from collections import Counter

import numpy as np
import pytest

import safegcd_model as model
import scalar_cases as sc
from oracle import p256
from test_algo_cpu import H, _w8  # noqa: F401  (H: the CPU build of the kernels' arithmetic)

N = sc.N

REACHABLE = {(s, p) for s in model.STATES for p in model.PATHS} - {(1, "rare-swap"), (2, "rare-swap"), (3, "rare-swap")}
WIDTHS = {(w, "e1") for w in range(1, 7)} | {(w, "i") for w in range(1, 7)} | {(6, "cap")}


def _from_w8(w):
    return sum(int(v) << 32 * i for i, v in enumerate(w))


@pytest.fixture(scope="module")
def edge_run():
    """_inv_wave (with the state machine in every batch) over S_EDGE, once:
    {s: (D, stats)}, the events reached"""
    events, out = set(), {}
    for _, _, s in sc.s_edge():
        st = {}
        D, batches = model._inv_wave(s, st, events)
        assert batches == st["batches"]
        out[s] = (D, st)
    return out, events


def test_s_edge_holds_every_class():
    edge = sc.s_edge()
    vals = [v for _, _, v in edge]
    assert len(vals) >= 1100 and len(set(vals)) == len(vals) and all(0 < v < N for v in vals)
    have = set(vals)
    want = [1, 2, 3, N - 1, N - 2, N - 3, (N - 1) // 2, (N + 1) // 2]
    want += [1 << k for k in range(256)] + [(1 << k) - 1 for k in range(2, 256)]
    want += [(1 << k) + 1 for k in range(1, 256)] + [N - (1 << k) for k in range(256)]
    want += [((1 << 261) - 1) % N]
    want += [x for _, _, x in sc.model_search()["picks"]]
    assert all(v in have for v in want)
    classes = Counter(c for c, _, _ in edge)
    assert classes["limb30"] == 32 and classes["limb30-all"] == 4 and classes["limb30-low"] == 2
    assert classes["word32"] == 16 and classes["random"] == 64 and classes["limb29"] == 2
    seams = {"2^29-1": (1 << 29) - 1, "2^29": 1 << 29, "2^29+1": (1 << 29) + 1, "2^30-1": sc.M30}
    for name, v in seams.items():
        for j in range(8):
            assert (sc.edge_value("limb %d = %s" % (j, name)) >> (30 * j)) & sc.M30 == v
        x = sc.edge_value("all limbs = %s" % name)
        assert all((x >> (30 * j)) & sc.M30 == v for j in range(8))
    assert sc.edge_value("low 30 bits zero") & sc.M30 == 0
    assert sc.edge_value("low 60 bits zero") & ((1 << 60) - 1) == 0 and sc.edge_value("low 60 bits zero") >> 60
    for j in range(8):
        for w in (0, 0xFFFFFFFF):
            assert (sc.edge_value("word %d = %08x" % (j, w)) >> (32 * j)) & 0xFFFFFFFF == w
    x = sc.edge_value("low eight 29-bit limbs = 2^29-1")
    assert x & ((1 << 232) - 1) == (1 << 232) - 1


def test_every_edge_inverse(H, edge_run):  # noqa: F811
    run, _ = edge_run
    out = (ctypes.c_uint32 * 8)()
    for _, label, s in sc.s_edge():
        want = pow(s, -1, N)
        for inv in (H.h_inv_n_words, H.h_inv_n_words_ct):
            inv(_w8(s), out)
            assert _from_w8(out) == want, label
        D, st = run[s]
        assert D % N == sc.R261 * want % N, label
        assert (D, st["batches"], st["max_eta"], st["max_d"]) == model.inv_stats(s), label


def test_state_machine_events(edge_run):
    """divsteps30_states agreed with _divsteps30_var on every batch of every
    S_EDGE inversion (it asserts that itself); S_EDGE reaches every (state,
    path) pair that any input can reach and every elimination width for every
    limiting term; random (eta, f, g) -- carried etas far from 0 too -- add
    nothing to the pairs."""
    _, events = edge_run
    assert {(e[0], e[1]) for e in events} == REACHABLE
    assert {(e[2], t) for e in events for t in e[3]} == WIDTHS
    for s in model.STATES:  # every state eliminates at the cap and below it
        ws = {e[2] for e in events if e[0] == s and e[2] is not None}
        assert ws == set(range(1, 7)), (s, ws)
    rng = random.Random(0xD1)
    more = set()
    for _ in range(4000):
        eta = rng.choice([-1, 0, 1, -2, 5, -30, 30, -241, 241, rng.randrange(-300, 300)])
        f, g = rng.getrandbits(32) | 1, rng.getrandbits(32) >> rng.choice([0, 0, 5, 17, 29, 32])
        model.divsteps30_states(eta, f, g, more)
    assert {(e[0], e[1]) for e in more} <= REACHABLE


def test_batch_counts(edge_run):
    """The histogram of the module docstring; the minimum is what
    inv_mod_n_wave's 14 untested batches assume (for speed, not correctness)."""
    run, _ = edge_run
    search = sc.model_search()
    hist = Counter(b for b, _, _ in search["stats"].values())
    print("batches over %d inputs: %s" % (len(search["stats"]), sorted(hist.items())))
    print("random alone: %s" % sorted(Counter(search["stats"][x][0] for x in set(search["random"])).items()))
    for _, label, x in search["picks"]:
        print("%s: %#x" % (label, x))
    counts = list(hist) + [st["batches"] for _, st in run.values()]
    assert min(counts) >= 15
    assert max(counts) <= 25
    assert hist == {16: 7, 17: 197, 18: 18598, 19: 2277}  # the docstring's figures (seeded)
    assert max(me for _, me, _ in search["stats"].values()) == 241
    assert max(md for _, _, md in search["stats"].values()) < 1.0


def test_construction_helpers():
    rng = random.Random(5)
    for k in (1, 2, N - 1, rng.randrange(N), rng.randrange(N)):
        assert sc.smul(k, p256.G) == p256.scalar_mult(k, p256.G)
    es, xs, ss = sc.grid_components()
    x = dict(xs)
    assert all(sc.lift_x(v) is not None and p256.on_curve(sc.lift_x(v)) for v in x.values())
    assert x["largest x < p-n"] < sc.P - N <= x["smallest x >= p-n"] < x["largest x < n"] < N
    assert N <= x["smallest x in [n, p)"] < x["largest x < p"] < sc.P
    # nothing on the curve lies between each pick and its bound
    assert not any(sc.usable_x(v) for v in range(0, x["smallest x"]))
    assert not any(sc.usable_x(v) for v in range(x["largest x < p-n"] + 1, sc.P - N))
    assert not any(sc.usable_x(v) for v in range(sc.P - N, x["smallest x >= p-n"]))
    assert not any(sc.usable_x(v) for v in range(x["largest x < n"] + 1, N))
    assert not any(sc.usable_x(v) for v in range(N, x["smallest x in [n, p)"]))
    assert not any(sc.usable_x(v) for v in range(x["largest x < p"] + 1, sc.P))
    assert [e for _, e in es][:7] == [0, 1, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1]
    assert es[7][1] < N <= es[8][1] < 1 << 256
    assert [s for _, s in ss][:4] == [1, N - 1, (N + 1) // 2, 1 << 255]


def _xy(key):
    return int.from_bytes(key[:32].tobytes(), "big"), int.from_bytes(key[32:].tobytes(), "big")


def _rs(sig):
    return int.from_bytes(sig[:32].tobytes(), "big"), int.from_bytes(sig[32:].tobytes(), "big")


def test_edge_signatures_under_both_oracles(oracle_lib):
    es = sc.edge_signatures()
    keys = sc.fixed_keys()[1]
    assert len(es["valid"]) == 2 * len(sc.s_edge()) and es["valid"].sum() == len(sc.s_edge())
    want = sc.oracle_keyed(oracle_lib, es["hashes"], es["sigs"], keys, es["kidx"])
    assert (want == es["valid"]).all(), [es["labels"][i] for i in np.nonzero(want != es["valid"])[0][:8]]
    qx, qy = _xy(keys[0])
    for i in range(len(es["valid"])):
        r, s = _rs(es["sigs"][i])
        assert s == es["s"][i]
        assert p256.verify(es["hashes"][i].tobytes(), r, s, qx, qy) == es["valid"][i], es["labels"][i]


def test_grid_signatures_under_both_oracles(oracle_lib):
    g = sc.grid()
    assert len(g["valid"]) == 648 and g["valid"].sum() == 324
    # (e and e + n give the same u1, hence the same key: 7 distinct e mod n, 7 x 36 keys)
    assert len({k.tobytes() for k in g["pubs"]}) == 252
    want = sc.oracle_own_key(oracle_lib, g["hashes"], g["sigs"], g["pubs"])
    assert (want == g["valid"]).all(), [g["labels"][i] for i in np.nonzero(want != g["valid"])[0][:8]]
    keys, kidx = sc.grid_registered()
    assert (sc.oracle_keyed(oracle_lib, g["hashes"], g["sigs"], keys, kidx) == g["valid"]).all()
    for i in range(len(g["valid"])):
        r, s = _rs(g["sigs"][i])
        assert p256.verify(g["hashes"][i].tobytes(), r, s, *_xy(g["pubs"][i])) == g["valid"][i], g["labels"][i]
    # the two x in [n, p): r = x - n, so the accepted candidate is r + n
    xs = dict(sc.grid_components()[1])
    rs = {_rs(sg)[0] for sg in g["sigs"][0::2]}
    assert xs["smallest x in [n, p)"] - N in rs and xs["largest x < p"] - N in rs


def test_h_scalars_on_every_chosen_s(H):  # noqa: F811
    """the CPU build of the scalar stage: u1 = e / s, u2 = r / s mod n"""
    es, g = sc.edge_signatures(), sc.grid()
    u1, u2 = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
    for src in (es, g):
        for i in np.nonzero(src["valid"])[0]:
            e = int.from_bytes(src["hashes"][i].tobytes(), "big")
            r, s = _rs(src["sigs"][i])
            assert H.h_scalars(_w8(e), _w8(r), _w8(s), u1, u2), src["labels"][i]
            w = pow(s, -1, N)
            assert _from_w8(u1) == e * w % N and _from_w8(u2) == r * w % N, src["labels"][i]


@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_groups(oracle_lib, K):
    G = sc.groups(K)
    n, L = G["n"], G["L"]
    assert n % (256 * K) != 0
    L2, lane, jj, grp = sc.ownership(K, n)
    assert L2 == L == 256 * -(-(-(-n // K)) // 256)
    # every signature lies in exactly one group
    seen = np.zeros(n, int)
    for gi in G["groups"]:
        seen[gi["members"]] += 1
        assert len(set(grp[gi["members"]].tolist())) == 1
        width = 64 if K <= 2 else 256
        assert len(gi["members"]) <= K * width and len(set((lane[gi["members"]] // width).tolist())) == 1
    assert (seen == 1).all()
    # the s of the arrays are the s of the bookkeeping; each group's total is its target
    svals = [_rs(sg)[1] for sg in G["sigs"]]
    assert svals == G["s"]
    targeted = [gi for gi in G["groups"] if gi["kind"] == "target"]
    assert len(targeted) >= (24 if K <= 2 else 8)
    for gi in G["groups"]:
        assert sc.group_total(svals[m] for m in gi["members"]) == gi["target"], gi["label"]
    tset = {gi["target"] for gi in targeted}
    assert all(t in tset for _, t in sc.required_targets()) and len(tset) == len(targeted)
    # members
    assert {v for _, _, v in sc.s_edge()} <= set(svals)
    special = {v for c, _, v in sc.s_edge() if c != "random"}
    for j in range(K):
        for ln in sc.SPECIAL_LANES:
            hit = [i for i in np.nonzero((jj == j) & (lane % 256 == ln))[0] if svals[i] in special]
            assert hit, (j, ln)
    kinds = np.array(G["kind"])
    n_out = [int((kinds[gi["members"]] == "out").sum()) for gi in targeted]
    assert sum(1 for c in n_out if c >= 3) >= 3
    assert all(not 0 < svals[i] < N for i in np.nonzero(kinds == "out")[0])
    broken = [set(kinds[gi["members"]].tolist()) & {"r=0", "r=n", "key"} for gi in targeted]
    assert sum(1 for b in broken if b) >= 2 and set().union(*broken) == {"r=0", "r=n", "key"}
    assert all(0 < svals[i] < N for i in np.nonzero(np.isin(kinds, ["r=0", "r=n", "key", "twin", "valid"]))[0])
    assert all(_rs(G["sigs"][i])[0] == 0 for i in np.nonzero(kinds == "r=0")[0])
    assert all(_rs(G["sigs"][i])[0] == N for i in np.nonzero(kinds == "r=n")[0])
    assert (G["kidx"][kinds == "key"] >= sc.N_KEYS).all() and (G["kidx"][kinds != "key"] < sc.N_KEYS).all()
    ones = [gi for gi in G["groups"] if gi["kind"] == "ones"]
    outs = [gi for gi in G["groups"] if gi["kind"] == "out"]
    assert len(ones) == 1 and all(svals[m] == 1 for m in ones[0]["members"]) and G["valid"][ones[0]["members"]].all()
    assert len(outs) == 1 and all(not 0 < svals[m] < N for m in outs[0]["members"])
    # the last block is ragged: its last lanes own one signature fewer
    assert len(G["groups"][-1]["members"]) < K * (64 if K <= 2 else 256) and G["groups"][-1]["kind"] == "target"
    # both oracles' verdicts: valid by construction <=> accepted
    want = sc.oracle_keyed(oracle_lib, G["hashes"], G["sigs"], sc.fixed_keys()[1], G["kidx"])
    assert (want == G["valid"]).all(), np.nonzero(want != G["valid"])[0][:8]
    assert G["valid"].sum() > 0.85 * n
    if K == 1:  # the Python oracle on the smallest batch's rejected members and a sample of the rest
        keys = sc.fixed_keys()[1]
        rng = random.Random(9)
        pick = [int(i) for i in np.nonzero(~G["valid"])[0]] + rng.sample(range(n), 60)
        for i in pick:
            k = int(G["kidx"][i])
            r, s = _rs(G["sigs"][i])
            got = k < sc.N_KEYS and p256.verify(G["hashes"][i].tobytes(), r, s, *_xy(keys[k]))
            assert got == G["valid"][i], (i, G["kind"][i])
