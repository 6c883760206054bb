"""k_sha256_ring (and the k_sha256 baseline) swept over every state of the
per-lane ring: every residue modulo 128 of the message's DEVICE address, every
length 0..704 (eleven blocks: the start-up, two ring periods, every tail at
every phase), and 80 long messages on both sides of the bucket clamp at 1024
compressions -- 90,320 messages in seeded random bytes (msgpath_cases.sha_sweep),
every digest against hashlib.

The data buffer is allocated first and the sweep is built for its address
residue, so the coverage the builder asserts speaks about the addresses the
kernel sees.  The sweep goes through pbftv_sha256_batch_dev with no order,
with the order pbftv_sha256_order_dev builds (plus expected digests and the
match bitmap) and with a random permutation (one wave then holds lanes of 1
to 3126 blocks), and through the host entry points (the DMA path).

PBFTV_SHA_RING=0 (k_sha256) is read once per process, so that kernel runs in
one fresh child process of this file."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import msgpath_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu


class Sweep:
    """The sweep resident on device 0, with hashlib's digests."""

    def __init__(self, ver):
        self.ver = ver
        self.d_data = ver.alloc(0, mc.sha_sweep_max_bytes() + 256)
        self.residue = self.d_data.ptr % 128
        self.blob, self.off, self.len = mc.sha_sweep(self.residue)
        self.n = n = len(self.len)
        assert ver._L.pbftv_memcpy_h2d(ver._h, 0, self.d_data.ptr, self.blob.ctypes.data, self.blob.nbytes) == 0
        self.want = mc.sha_expected(self.blob, self.off, self.len)
        self.flip = np.arange(n) % 3 == 0  # expected digests with one bit wrong
        exp = self.want.copy()
        exp[self.flip, 31] ^= 0x10
        self.exp = exp
        self.d_off, self.d_len = ver.to_device(0, self.off), ver.to_device(0, self.len)
        self.d_exp = ver.to_device(0, exp)
        self.d_ord, self.d_dig, self.d_bm = ver.alloc(0, 4 * n), ver.alloc(0, 32 * n), ver.alloc(0, (n + 31) // 32 * 4)

    def run(self, order, expected: bool):
        """One pbftv_sha256_batch_dev call: (digests, match bits | None)."""
        v = self.ver
        self.d_dig.zero()
        self.d_bm.zero()
        v.sha256_batch_dev(0, self.d_data.ptr, self.d_off.ptr, self.d_len.ptr, order, self.n, self.d_dig.ptr,
                           self.d_exp.ptr if expected else None, self.d_bm.ptr if expected else None)
        v.sync(0)
        got = self.d_dig.to_host().reshape(self.n, 32)
        bits = np.unpackbits(self.d_bm.to_host(), bitorder="little")[:self.n].astype(bool) if expected else None
        return got, bits

    def wrong(self, got) -> list:
        """(address residue, length) of the first messages whose digest differs."""
        bad = np.nonzero((got != self.want).any(1))[0]
        return [((self.residue + int(self.off[i])) % 128, int(self.len[i])) for i in bad[:12]]

    def no_order(self):
        got, _ = self.run(None, False)
        return self.wrong(got)

    def device_order(self):
        """The order pbftv_sha256_order_dev builds: what is wrong with it, wrong digests, wrong bits."""
        v, n = self.ver, self.n
        v.sha256_order_dev(0, self.d_len.ptr, n, self.d_ord.ptr)
        got, bits = self.run(self.d_ord.ptr, True)
        order = self.d_ord.to_host(dtype=np.uint32).astype(np.int64)
        faults = []
        if not (np.sort(order) == np.arange(n)).all():
            faults.append("not a permutation")
        else:
            nb = mc.sha_blocks(self.len)[order]  # (clamped: 1023 to 3126 compressions share a bucket)
            if not (np.diff(nb) <= 0).all():
                faults.append("block counts increase along the order")
        wrong_bits = np.nonzero(bits != ~self.flip)[0]
        return faults, self.wrong(got), [(int(i), int(self.len[i])) for i in wrong_bits[:12]]

    def free(self):
        for b in (self.d_data, self.d_off, self.d_len, self.d_exp, self.d_ord, self.d_dig, self.d_bm):
            b.free()


@pytest.fixture(scope="module")
def ver():
    from simple_pbft_amd import Verifier
    v = Verifier()
    yield v
    v.close()


@pytest.fixture(scope="module")
def sweep(ver):
    s = Sweep(ver)
    print(f"[sha sweep] device buffer residue {s.residue}, {s.n} messages, {s.blob.nbytes} bytes")
    yield s
    s.free()


def test_sweep_speaks_about_device_addresses(sweep):
    addr = (sweep.d_data.ptr + sweep.off.astype(np.int64)) % 128
    seen = set(zip(addr.tolist(), sweep.len.tolist()))
    assert all((r, k) in seen for r in range(128) for k in range(705))
    assert sweep.n % 32 and sweep.n % 64 and sweep.n % 256


def test_every_digest_without_order(sweep):
    assert sweep.no_order() == []


def test_device_order_digests_and_bits(sweep):
    faults, wrong, wrong_bits = sweep.device_order()
    assert faults == [] and wrong == [] and wrong_bits == []


def test_random_permutation_as_order(sweep):
    """Lanes of 1 to 3126 blocks side by side in one wave."""
    perm = np.random.default_rng(0x0DE5).permutation(sweep.n).astype(np.uint32)
    d_perm = sweep.ver.to_device(0, perm)
    try:
        got, bits = sweep.run(d_perm.ptr, True)
    finally:
        d_perm.free()
    assert sweep.wrong(got) == []
    assert (bits == ~sweep.flip).all()


def test_host_entry_points(ver, sweep):
    """pbftv_sha256_batch and pbftv_digest_check_batch on the same blob: the
    DMA path, which always takes the block-count order."""
    got = ver.sha256_batch(sweep.blob, sweep.off, sweep.len)
    assert sweep.wrong(got) == []
    bits = ver.digest_check_batch(sweep.blob, sweep.off, sweep.len, sweep.exp)
    assert (bits == ~sweep.flip).all()


def baseline() -> int:
    """The first two runs under whatever kernel this process selected; 0 when all is right."""
    from simple_pbft_amd import Verifier
    with Verifier(device_mask=1) as v:
        s = Sweep(v)
        wrong = s.no_order()
        faults, wrong2, wrong_bits = s.device_order()
        s.free()
    print(f"[sha sweep] residue {s.residue}")
    if wrong or faults or wrong2 or wrong_bits:
        print(f"no order: wrong (residue, len) {wrong}\ndevice order: {faults}, wrong (residue, len) {wrong2}, "
              f"wrong bits (message, len) {wrong_bits}")
        return 1
    return 0


def test_dword_window_kernel_in_a_fresh_process():
    """PBFTV_SHA_RING=0 selects k_sha256, the A/B baseline of the ring kernel."""
    env = dict(os.environ, PBFTV_SHA_RING="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "baseline"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    if sys.argv[1:] != ["baseline"]:
        raise SystemExit(f"unknown mode {sys.argv[1:]}")
    raise SystemExit(baseline())
