"""Keys in SEC1 wire form for tests/test_sec1_cpu.py, tests/test_gpu_wirekey.py
and tests/test_gpu_flush_wirekey.py: the Python big-integer decode that every
expected value comes from (SEC1 2.3.3 / 2.3.4 as go1.19 elliptic.Unmarshal /
UnmarshalCompressed apply them), encoders, the rejected-encoding set, and the
expected bits -- the oracle's verdict under the key Python decodes, 0 where
Python rejects the key."""
from __future__ import annotations

import json
import os

import numpy as np

from conftest import GOLDEN, oracle_sign_pool

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
GX = 0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296
GY = 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5

KEY_XY, KEY_COMPRESSED, KEY_UNCOMPRESSED = 0, 1, 2
STRIDE = {KEY_XY: 64, KEY_COMPRESSED: 33, KEY_UNCOMPRESSED: 65}

_cache: dict = {}


def rhs(x: int) -> int:
    return (x * x * x - 3 * x + B) % P


def sqrt_p(t: int):
    """(y, is a root) with y = t^((p+1)/4): the root the device must find."""
    y = pow(t, (P + 1) // 4, P)
    return y, y * y % P == t % P


def on_curve(x: int, y: int) -> bool:
    return 0 <= x < P and 0 <= y < P and y * y % P == rhs(x)


def decode(key: bytes, fmt: int):
    """(x, y) or None: the reference decode in Python big integers."""
    key = bytes(key)
    assert len(key) == STRIDE[fmt]
    if fmt == KEY_XY:
        x, y = int.from_bytes(key[:32], "big"), int.from_bytes(key[32:], "big")
        return (x, y) if on_curve(x, y) else None
    if fmt == KEY_UNCOMPRESSED:
        if key[0] != 4:
            return None
        x, y = int.from_bytes(key[1:33], "big"), int.from_bytes(key[33:], "big")
        return (x, y) if on_curve(x, y) else None
    if key[0] not in (2, 3):
        return None
    x = int.from_bytes(key[1:], "big")
    if x >= P:
        return None
    y, ok = sqrt_p(rhs(x))
    if not ok:
        return None
    if (y & 1) != (key[0] & 1):
        y = P - y
    return x, y


def xy_bytes(x: int, y: int) -> bytes:
    return x.to_bytes(32, "big") + y.to_bytes(32, "big")


def encode_one(xy: bytes, fmt: int, wrong_parity: bool = False) -> bytes:
    """One X||Y key in fmt.  A key that is no point keeps its bytes (compressed:
    its X and Y's parity), so it is rejected or lands on another point."""
    xy = bytes(xy)
    if fmt == KEY_XY:
        return xy
    if fmt == KEY_UNCOMPRESSED:
        return b"\x04" + xy
    return bytes([2 + ((xy[63] & 1) ^ (1 if wrong_parity else 0))]) + xy[:32]


def encode(pubs: np.ndarray, fmt: int) -> np.ndarray:
    """pubs (n, 64) -> (n, stride) uint8, packed."""
    pubs = np.ascontiguousarray(pubs, np.uint8).reshape(-1, 64)
    out = np.zeros((len(pubs), STRIDE[fmt]), np.uint8)
    if fmt == KEY_XY:
        out[:] = pubs
    elif fmt == KEY_UNCOMPRESSED:
        out[:, 0] = 4
        out[:, 1:] = pubs
    else:
        out[:, 0] = 2 + (pubs[:, 63] & 1)
        out[:, 1:] = pubs[:, :32]
    return out


def decoded_xy(keys: np.ndarray, fmt: int):
    """Python's decode of every key: (xy (n, 64) with zeros where rejected, accepted mask)."""
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, STRIDE[fmt])
    xy = np.zeros((len(keys), 64), np.uint8)
    ok = np.zeros(len(keys), bool)
    memo: dict = {}
    for i, k in enumerate(keys):
        kb = k.tobytes()
        if kb not in memo:
            memo[kb] = decode(kb, fmt)
        if memo[kb] is not None:
            xy[i] = np.frombuffer(xy_bytes(*memo[kb]), np.uint8)
            ok[i] = True
    return xy, ok


def expect(oracle_lib, hashes, sigs, keys, fmt) -> np.ndarray:
    """The oracle's verdict for signature i under Python's decode of key i; 0
    where Python rejects the key.  Equal (hash, sig, key) triples are asked once."""
    hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
    sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 64)
    xy, ok = decoded_xy(keys, fmt)
    out = np.zeros(len(hashes), bool)
    memo: dict = {}
    for i in range(len(hashes)):
        if not ok[i]:
            continue
        k = (hashes[i].tobytes(), sigs[i].tobytes(), xy[i].tobytes())
        if k not in memo:
            memo[k] = oracle_lib.oracle_ecdsa_p256_verify(hashes[i].ctypes.data, sigs[i].ctypes.data,
                                                          xy[i].ctypes.data) == 1
        out[i] = memo[k]
    return out


def golden_keys():
    """The fixture's key list as (xy bytes, valid)."""
    with open(os.path.join(GOLDEN, "ecdsa.json")) as f:
        fx = json.load(f)
    return [(bytes.fromhex(k["x"]) + bytes.fromhex(k["y"]), bool(k["valid"])) for k in fx["keys"]]


def rejected_set(oracle_lib):
    """One valid signature under one valid key, then that signature under every
    encoding the issue lists.  (name, fmt, key bytes) -- hashes and sigs are the
    same for all.  Returns hash (32,), sig (64,), the key's xy, the list."""
    if "rej" in _cache:
        return _cache["rej"]
    keys, hashes, sigs, _ = oracle_sign_pool(oracle_lib, 1, 1, seed=3311)
    xy = keys[0].tobytes()
    x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:], "big")
    assert on_curve(x, y)
    good_c, good_u = encode_one(xy, KEY_COMPRESSED), encode_one(xy, KEY_UNCOMPRESSED)
    cases = [("compressed, right prefix", KEY_COMPRESSED, good_c),
             ("compressed, wrong parity", KEY_COMPRESSED, encode_one(xy, KEY_COMPRESSED, wrong_parity=True)),
             ("compressed, X = p", KEY_COMPRESSED, b"\x02" + P.to_bytes(32, "big")),
             ("compressed, X = 2^256 - 1", KEY_COMPRESSED, b"\x03" + b"\xff" * 32),
             ("uncompressed, right prefix", KEY_UNCOMPRESSED, good_u),
             ("uncompressed, Y = p", KEY_UNCOMPRESSED, b"\x04" + xy[:32] + P.to_bytes(32, "big")),
             ("uncompressed, Y = 2^256 - 1", KEY_UNCOMPRESSED, b"\x04" + xy[:32] + b"\xff" * 32),
             ("uncompressed, X = p", KEY_UNCOMPRESSED, b"\x04" + P.to_bytes(32, "big") + xy[32:]),
             ("uncompressed, y negated", KEY_UNCOMPRESSED, b"\x04" + xy_bytes(x, P - y))]
    for pre in (0x00, 0x01, 0x04, 0x05, 0x06, 0x07, 0xFF):
        cases.append(("compressed, prefix %02x" % pre, KEY_COMPRESSED, bytes([pre]) + xy[:32]))
    for pre in (0x00, 0x02, 0x03, 0x06, 0x07):
        cases.append(("uncompressed, prefix %02x" % pre, KEY_UNCOMPRESSED, bytes([pre]) + xy))
    # an X with no point at all (about half of them): under both prefixes
    xn = next(v for v in range(x + 1, x + 200) if not sqrt_p(rhs(v))[1])
    cases.append(("compressed, X without a point (02)", KEY_COMPRESSED, b"\x02" + xn.to_bytes(32, "big")))
    cases.append(("compressed, X without a point (03)", KEY_COMPRESSED, b"\x03" + xn.to_bytes(32, "big")))
    for kxy, valid in golden_keys():
        if not valid:
            cases.append(("uncompressed, off-curve fixture key", KEY_UNCOMPRESSED, b"\x04" + kxy))
    _cache["rej"] = (hashes[0], sigs[0], keys[0], cases)
    return _cache["rej"]


def spread(oracle_lib, fmt: int, n: int, every: int = 3):
    """n signatures in fmt: the valid (hash, sig, key) of rejected_set, and at
    every `every`-th place one of the set's encodings of that format in turn,
    so that each wave holds accepted and rejected keys side by side.
    Returns hashes, sigs, keys (n, stride), expect."""
    h0, s0, xy, cases = rejected_set(oracle_lib)
    mine = [k for _, f, k in cases if f == fmt]
    good = encode_one(xy.tobytes(), fmt)
    rows = [mine[(i // every) % len(mine)] if i % every == every - 1 else good for i in range(n)]
    keys = np.frombuffer(b"".join(rows), np.uint8).reshape(n, STRIDE[fmt]).copy()
    hashes, sigs = np.tile(h0, (n, 1)), np.tile(s0, (n, 1))
    return hashes, sigs, keys, expect(oracle_lib, hashes, sigs, keys, fmt)
