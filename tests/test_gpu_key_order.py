"""The key-order stage of the lane path (k_key_hist, the scatter inside
k_ecdsa_scalars, the comb's result bytes, k_pack_bits) at its edges, small and
fast: key counts across the 256-thread scan's groups of 5 bins and at the
1,024-key limit, degenerate histograms, every K (signatures per lane) with more
bins than the block inversion borrows, runs of batches that alternate the
header's two counter sets, and the sizes one below the default rule's
thresholds.

Every case is bit-exact against oracle_ecdsa_p256_verify_batch on whole bitmap
bytes (padding bits past n must be 0, the bytes after the bitmap untouched),
except the tiled sizes of test 5, which use the corruption mask over the
oracle-signed pool.  Each test also asserts through pbftv_lib_counters how many
batches took the key order.

One pool per module: 1,025 keys x 3 signatures from the oracle's signer; the
tests register prefixes of the key set at the cheapest geometry (8-bit windows,
270 KB per key)."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import oracle_sign_pool

pytestmark = pytest.mark.gpu

POOL_KEYS, PER_KEY = 1025, 3
N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
GUARD = 16  # bytes after each bitmap that no kernel may touch


@pytest.fixture(autouse=True)
def geometry(monkeypatch):
    monkeypatch.setenv("PBFTV_GBITS", "8")
    monkeypatch.setenv("PBFTV_QBITS", "8")
    monkeypatch.setenv("PBFTV_WAVE_MAX", "0")
    monkeypatch.setenv("PBFTV_KEY_SORT", "1")
    monkeypatch.delenv("PBFTV_SCALAR_BATCH", raising=False)


@pytest.fixture(scope="module")
def signed(oracle_lib):
    keys, H, S, K = oracle_sign_pool(oracle_lib, n_keys=POOL_KEYS, per_key=PER_KEY, seed=0x4B4F)
    for a in (keys, H, S, K):
        a.setflags(write=False)
    return keys, H, S, K


@pytest.fixture(scope="module")
def ver():
    from simple_pbft_amd import Verifier
    v = Verifier(device_mask=1)
    yield v
    v.close()


def corrupt(H, S, K, nkeys, frac, rng, move_keys=True):
    """The usual classes on a `frac` subset, in place: a bit of r, of s, of the
    hash, another registered key (move_keys; else the hash again), r = 0, s = 0,
    r = n, s = 0xFF.."""
    n = len(K)
    idx = rng.choice(n, int(round(n * frac)), replace=False)
    nb = np.frombuffer(N_ORDER.to_bytes(32, "big"), np.uint8)
    for t, i in enumerate(idx):
        c = t % 8
        if c == 0:
            S[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == 1:
            S[i, 32 + rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == 2 or (c == 3 and (nkeys == 1 or not move_keys)):
            H[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == 3:
            K[i] = (K[i] + 1 + rng.integers(0, nkeys - 1)) % nkeys
        elif c == 4:
            S[i, :32] = 0
        elif c == 5:
            S[i, 32:] = 0
        elif c == 6:
            S[i, :32] = nb
        else:
            S[i, 32:] = 0xFF


def draw(signed, n, nkeys, seed, *, on_key=None, one_per_key=False, all_out=False, out_frac=0.02, frac=0.2):
    """A batch of n from the pool's signatures of keys < nkeys, corrupted:
    uniform over the keys with out-of-range key indices among them, or every
    key index out of range, or (key indices then stay as drawn) all on one key
    or exactly one per key."""
    _, PH, PS, PK = signed
    rng = np.random.default_rng(seed)
    fixed_keys = one_per_key or on_key is not None
    if one_per_key:
        assert n == nkeys
        pick = rng.permutation(nkeys) * PER_KEY + rng.integers(0, PER_KEY, nkeys)
    elif on_key is not None:
        pick = on_key * PER_KEY + rng.integers(0, PER_KEY, n)
    else:
        pick = rng.integers(0, nkeys * PER_KEY, n)
    H, S, K = PH[pick].copy(), PS[pick].copy(), PK[pick].copy()
    corrupt(H, S, K, nkeys, frac, rng, move_keys=not fixed_keys)
    if fixed_keys:
        assert (K == on_key).all() if on_key is not None else sorted(K.tolist()) == list(range(nkeys))
    elif all_out:
        K[:] = nkeys + rng.integers(0, 5000, n)
        K[0], K[-1] = nkeys, 0xFFFFFFFF
    elif out_frac:
        K[rng.random(n) < out_frac] = nkeys + rng.integers(0, 1000)
    return H, S, K


def oracle_bytes(oracle_lib, keys, H, S, K):
    n = len(K)
    want = np.zeros((n + 7) // 8, np.uint8)
    keys = np.ascontiguousarray(keys)
    oracle_lib.oracle_ecdsa_p256_verify_batch(H.ctypes.data, S.ctypes.data, K.ctypes.data, n, keys.ctypes.data,
                                              len(keys), want.ctypes.data, 16)
    bits = np.unpackbits(want, bitorder="little")[:n]
    return np.packbits(bits, bitorder="little")  # (whole bytes, padding bits 0)


class Batch:
    """A batch's own device buffers; the bitmap starts as 0xFF, guard included."""

    def __init__(self, v, H, S, K):
        self.v, self.n = v, len(K)
        self.nb = (self.n + 7) // 8
        self.bufs = [v.to_device(0, a) for a in (H, S, np.ascontiguousarray(K, np.uint32))]
        self.bm = v.alloc(0, self.nb + GUARD)
        assert v._L.pbftv_memset_dev(v._h, 0, self.bm.ptr, 0xFF, self.nb + GUARD) == 0

    def enqueue(self, stream=None):
        h, s, k = self.bufs
        self.v.verify_batch_dev(0, h.ptr, s.ptr, k.ptr, self.n, self.bm.ptr, stream=stream)

    def result(self):
        raw = self.bm.to_host()
        assert (raw[self.nb:] == 0xFF).all(), "bytes after the bitmap were written"
        return raw[:self.nb]

    def free(self):
        for b in self.bufs + [self.bm]:
            b.free()


def sorted_batches(v):
    c = v.lib_counters(0)
    assert c["held_events"] + c["spare_events"] == c["events_created"]
    return c["sorted_batches"]


def check_one(v, oracle_lib, keys, H, S, K, what, *, sorts=1, accept=None):
    before = sorted_batches(v)
    b = Batch(v, H, S, K)
    try:
        b.enqueue()
        v.sync(0)
        got = b.result()
    finally:
        b.free()
    want = oracle_bytes(oracle_lib, keys, H, S, K)
    diff = np.unpackbits(got ^ want, bitorder="little")
    assert not diff.any(), f"{what}: {int(diff.sum())} bits differ, first at {int(np.argmax(diff))} of {len(K)}"
    assert sorted_batches(v) - before == sorts, what
    if accept is not None:
        rate = np.unpackbits(want, bitorder="little")[:len(K)].mean()
        assert accept[0] <= rate <= accept[1], (what, rate)  # the case tests what it says


# ---------------------------------------------------------------- 1: key counts
@pytest.mark.parametrize("nkeys", [1, 8, 9, 255, 256, 257, 1023, 1024])
def test_key_counts(ver, oracle_lib, signed, nkeys):
    """2,999 signatures spread over 1 .. 1,024 keys: one bin, bins that end
    inside / on / after a thread's group of 5 in the block scan, the limit."""
    keys = signed[0][:nkeys]
    assert ver.register_keys(keys).all()
    H, S, K = draw(signed, 2999, nkeys, seed=1000 + nkeys)
    check_one(ver, oracle_lib, keys, H, S, K, f"{nkeys} keys", accept=(0.7, 0.85))


def test_1025_keys_refuse_the_sort(ver, oracle_lib, signed):
    """One key past kSortMaxKeys: arrival order, the key order not taken, still exact."""
    keys = signed[0][:1025]
    assert ver.register_keys(keys).all()
    H, S, K = draw(signed, 2999, 1025, seed=2025)
    check_one(ver, oracle_lib, keys, H, S, K, "1025 keys", sorts=0, accept=(0.7, 0.85))


# ---------------------------------------------------------------- 2: histograms at 257 keys
SIZES = [1, 63, 64, 65, 255, 256, 257, 2999]


@pytest.mark.parametrize("shape", ["key 0", "key 256", "all out of range", "one per key", "key off the curve"])
def test_histograms_at_257_keys(ver, oracle_lib, signed, shape):
    keys = signed[0][:257].copy()
    if shape == "key off the curve":
        keys[128, 63] ^= 1
    assert ver.register_keys(keys).tolist() == [not (shape == "key off the curve" and j == 128) for j in range(257)]
    for n in ([257] if shape == "one per key" else SIZES):
        kw, accept = {}, None
        if shape == "key 0":
            kw = dict(on_key=0)
        elif shape == "key 256":
            kw = dict(on_key=256)
        elif shape == "all out of range":
            kw, accept = dict(all_out=True), (0.0, 0.0)
        elif shape == "one per key":
            kw, accept = dict(one_per_key=True), (0.7, 0.9)
        H, S, K = draw(signed, n, 257, seed=3000 + n, **kw)
        if shape == "key off the curve" and n >= 255:
            assert (K == 128).any()
        check_one(ver, oracle_lib, keys, H, S, K, f"{shape}, n = {n}", accept=accept)


# ---------------------------------------------------------------- 3: signatures per lane
@pytest.fixture(scope="module")
def batch_600(oracle_lib, signed):
    H, S, K = draw(signed, 5000, 600, seed=4600)
    return H, S, K, oracle_bytes(oracle_lib, signed[0][:600], H, S, K)


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_signatures_per_lane_under_a_key_order(ver, signed, batch_600, k, monkeypatch):
    """600 keys = 601 bins, more than the 576 words of kstart[] the block
    inversion (K >= 4) borrows after the claims; n = 5,000 is no multiple of
    256 K for any K, so the last lanes hold fewer than K signatures."""
    monkeypatch.setenv("PBFTV_SCALAR_BATCH", str(k))
    H, S, K, want = batch_600
    assert ver.register_keys(signed[0][:600]).all()
    before = sorted_batches(ver)
    b = Batch(ver, H, S, K)
    try:
        b.enqueue()
        ver.sync(0)
        got = b.result()
    finally:
        b.free()
    diff = np.unpackbits(got ^ want, bitorder="little")
    assert not diff.any(), f"K = {k}: {int(diff.sum())} bits differ, first at {int(np.argmax(diff))}"
    assert sorted_batches(ver) - before == 1
    assert 0.7 < np.unpackbits(want, bitorder="little")[:5000].mean() < 0.85


# ---------------------------------------------------------------- 4: consecutive batches
RUN = [  # (keys registered, n, draw arguments)
    (257, 2999, {}),
    (257, 64, dict(on_key=256)),
    (257, 257, dict(one_per_key=True)),
    (257, 1, {}),
    (257, 2999, dict(all_out=True)),
    (257, 1000, {}),
    (9, 500, {}),
    (9, 8, {}),
    (1024, 2999, {}),
]


@pytest.fixture(scope="module")
def run_inputs(oracle_lib, signed):
    out = []
    for j, (nkeys, n, kw) in enumerate(RUN):
        H, S, K = draw(signed, n, nkeys, seed=5000 + j, **kw)
        out.append((H, S, K, oracle_bytes(oracle_lib, signed[0][:nkeys], H, S, K)))
    return out


@pytest.mark.parametrize("where", ["context stream", "library stream"])
def test_consecutive_batches_alternate_the_counter_sets(ver, signed, run_inputs, where):
    """Nine batches back to back on one stream and one scratch, sizes and key
    sets shrinking and growing, no bitmap read and no host wait of the test's
    own until the end: a total or a claim left over from two batches back (the
    header's other counter set) would misplace records."""
    stream = ver.stream_create(0) if where == "library stream" else None
    assert ver.register_keys(signed[0][:RUN[0][0]]).all()
    batches = [Batch(ver, H, S, K) for H, S, K, _ in run_inputs]  # (every upload before the first batch)
    before = sorted_batches(ver)
    try:
        registered = RUN[0][0]
        for b, (nkeys, _, _) in zip(batches, RUN):
            if nkeys != registered:  # (waits for this context's verifies in flight, reads nothing back)
                assert ver.register_keys(signed[0][:nkeys]).all()
                registered = nkeys
            b.enqueue(stream)
        if stream is None:
            ver.sync(0)
        else:
            ver.stream_wait(0, stream)
        for j, (b, (_, _, _, want)) in enumerate(zip(batches, run_inputs)):
            diff = np.unpackbits(b.result() ^ want, bitorder="little")
            assert not diff.any(), f"batch {j} {RUN[j]}: {int(diff.sum())} bits differ, first at {int(np.argmax(diff))}"
        assert sorted_batches(ver) - before == len(RUN)
    finally:
        if stream is not None:
            ver.stream_destroy(0, stream)
        for b in batches:
            b.free()


# ---------------------------------------------------------------- 5: below the thresholds
def tiled_case(signed, n, nkeys, seed):
    """n signatures tiled from the pool's signatures of keys < nkeys in random
    order, 1 % with one bit of s flipped: the accept bits are the complement."""
    _, PH, PS, PK = signed
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, nkeys * PER_KEY, n)
    H, S, K = PH[pick], PS[pick].copy(), PK[pick]
    bad = rng.random(n) < 0.01
    S[np.nonzero(bad)[0], 63] ^= 1
    return np.ascontiguousarray(H), S, np.ascontiguousarray(K), ~bad


@pytest.mark.parametrize("n,nkeys,sorts", [(32767, 8, 0), (32767, 9, 0), (32768, 8, 0), (32768, 9, 1),
                                           (131071, 100, 1), (262143, 100, 1)])
def test_default_rule_just_below_the_thresholds(ver, signed, n, nkeys, sorts, monkeypatch):
    """PBFTV_KEY_SORT unset: the key order from 9 keys and 32,768 signatures on;
    131,071 (K = 1) and 262,143 (K = 2) are ragged, n % 8 = 7, with a partial
    last block."""
    monkeypatch.delenv("PBFTV_KEY_SORT")
    assert ver.register_keys(signed[0][:nkeys]).all()
    H, S, K, ok = tiled_case(signed, n, nkeys, seed=6000 + n + nkeys)
    before = sorted_batches(ver)
    b = Batch(ver, H, S, K)
    try:
        b.enqueue()
        ver.sync(0)
        got = b.result()
    finally:
        b.free()
    diff = np.unpackbits(got ^ np.packbits(ok, bitorder="little"), bitorder="little")
    assert not diff.any(), f"n = {n}, {nkeys} keys: {int(diff.sum())} bits differ, first at {int(np.argmax(diff))}"
    assert sorted_batches(ver) - before == sorts
