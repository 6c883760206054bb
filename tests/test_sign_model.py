"""tests/rfc6979_model.py, the reference every signer test compares with, pinned
on the two P-256 / SHA-256 rows of RFC 6979 §A.2.5 that tests/golden/ecdsa.json
already holds (key C9AFA9D8...0F6721, messages "sample" and "test")."""
from __future__ import annotations

import hashlib

import rfc6979_model as model
from oracle import p256

RFC_KEY = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
RFC_K = {b"sample": 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
         b"test": 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0}


def _rows(ecdsa_fixtures):
    rows = [v for v in ecdsa_fixtures["vectors"] if v["kind"].startswith("rfc6979") and v["expect"]]
    by_hash = {v["hash"]: v for v in rows}
    return [(m, by_hash[hashlib.sha256(m).hexdigest()]) for m in (b"sample", b"test")]


def test_model_reproduces_the_rfc_rows(ecdsa_fixtures):
    key = ecdsa_fixtures["keys"][0]
    assert p256.pubkey(RFC_KEY) == (int(key["x"], 16), int(key["y"], 16))
    for msg, v in _rows(ecdsa_fixtures):
        h = hashlib.sha256(msg).digest()
        assert v["key"] == 0
        k, j = model.nonce(RFC_KEY, h)
        assert (k, j) == (RFC_K[msg], 0)
        r, s = model.sign(h, RFC_KEY)
        assert (f"{r:064x}", f"{s:064x}") == (v["r"], v["s"])
        assert model.sign_bytes(h, RFC_KEY).hex() == v["r"] + v["s"]
        assert p256.verify(h, r, s, *p256.pubkey(RFC_KEY))


def test_bits2octets_and_the_refusals():
    n = p256.N
    assert model.bits2octets(n.to_bytes(32, "big")) == bytes(32)
    assert model.bits2octets((n - 1).to_bytes(32, "big")) == (n - 1).to_bytes(32, "big")
    assert model.bits2octets(b"\xff" * 32) == ((1 << 256) - 1 - n).to_bytes(32, "big")
    for d in (0, n, (1 << 256) - 1):
        assert model.sign(bytes(32), d) is None and model.sign_bytes(bytes(32), d) == bytes(64)
    # successive candidates differ and the generator is a pure function of (d, h1)
    g1, g2 = model.candidates(5, bytes(32)), model.candidates(5, bytes(32))
    a = [next(g1) for _ in range(3)]
    assert a == [next(g2) for _ in range(3)] and len(set(a)) == 3
