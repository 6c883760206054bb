"""Deterministic ECDSA-P256 signing as the reference for sign.h: the HMAC-SHA256
DRBG of RFC 6979 §3.2 for qlen = hlen = 256 (the candidate generator) on top
of hmac / hashlib, and the signature itself through oracle.p256.sign.  No
low-S normalisation (Go's ecdsa.Sign does none).  Pure Python, test-only."""
from __future__ import annotations

import hashlib
import hmac

from oracle import p256

N = p256.N
MAX_CANDIDATES = 4  # sign.h's bound; the model reports None past it, as the product writes zeros


def bits2octets(h1: bytes) -> bytes:
    """§2.3.4 for qlen = 256: the 32-byte hash as an integer, minus n when >= n."""
    z = int.from_bytes(h1, "big")
    return (z - N if z >= N else z).to_bytes(32, "big")


def candidates(d: int, h1: bytes):
    """The successive T values of §3.2 step h as integers (an endless generator);
    the caller keeps the first with 0 < k < n."""
    assert len(h1) == 32
    x = d.to_bytes(32, "big")
    h = bits2octets(h1)
    mac = lambda key, msg: hmac.new(key, msg, hashlib.sha256).digest()
    V, K = b"\x01" * 32, b"\x00" * 32
    K = mac(K, V + b"\x00" + x + h)
    V = mac(K, V)
    K = mac(K, V + b"\x01" + x + h)
    V = mac(K, V)
    while True:
        V = mac(K, V)
        yield int.from_bytes(V, "big")
        K = mac(K, V + b"\x00")
        V = mac(K, V)


def nonce(d: int, h1: bytes):
    """(k, index of the candidate taken) or None past MAX_CANDIDATES."""
    for j, k in zip(range(MAX_CANDIDATES), candidates(d, h1)):
        if 0 < k < N:
            return k, j
    return None


def sign_with_k(h1: bytes, d: int, k: int):
    """(r, s) for the explicit nonce k, or None where r or s is zero."""
    try:
        return p256.sign(h1, d, k)
    except ValueError:
        return None


def sign(h1: bytes, d: int):
    """(r, s) as ecdsa_sign computes it, or None (then the product writes 64
    zero bytes and a 0 ok bit): d out of range, or no candidate in 4 signs."""
    if not 0 < d < N:
        return None
    for j, k in zip(range(MAX_CANDIDATES), candidates(d, h1)):
        if 0 < k < N:
            rs = sign_with_k(h1, d, k)
            if rs is not None:
                return rs
    return None


def sign_bytes(h1: bytes, d: int) -> bytes:
    rs = sign(h1, d)
    return bytes(64) if rs is None else rs[0].to_bytes(32, "big") + rs[1].to_bytes(32, "big")
