"""The case set of the Schnorr verifier tests: plain Python integers over the runtime's G1 bindings.

A valid signature with a CHOSEN r exists only under a key made for it: pick a nonce v, T = v G, c = H(T, m) with the
host's blake2xb, then sk = (v - r) / c mod n and pk = sk G give r G + c pk = v G.  So every chosen-r case brings
its own key; the ordinary cases, the chosen top bytes of c (found by trying nonces) and the invalid cases share
eight ordinary keys.  Built once per process (cases()), never modified.

Expected status: 0 valid | 1 c >= n or r >= n | 2 challenge differs | 4 an index out of range (the host verifier
has no indices: those cases are not cross-checked).  Status 3 (the draw cap) must not occur: test_schnorr_cases_cpu
checks that no case needs more than DRAWS candidates.
"""
from __future__ import annotations

import random
from typing import NamedTuple

from biscotti_amd.native import rt

DRAWS = 32


class Case(NamedTuple):
    name: str
    msg_idx: int
    key_idx: int
    sig: bytes
    expect: int


def be32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def challenge(tm: bytes, msg: bytes, limit: int = 64):
    """hash_schnorr with plain integers: (c, candidates drawn)."""
    R = rt()
    n = R.bn256_order()
    stream = R.blake2xb(tm, msg, 32 * limit)
    for j in range(limit):
        v = int.from_bytes(stream[32 * j:32 * j + 32], "big")
        if 0 < v < n:
            return v, j + 1
    raise AssertionError("no candidate in %d draws" % limit)


def point(r: int, c: int, pk: bytes) -> bytes:
    """marshal(r G + c PK) by the host."""
    R = rt()
    return R.g1_add(R.g1_base_mul(r), R.g1_mul(pk, c))


_CACHE = None


def cases():
    """dict: keys (64-byte marshals, key index = position), messages (64 bytes each), cases [Case], scalars
    [(r, c, key_idx)] -- the edge scalars of the point-sum test."""
    global _CACHE
    if _CACHE is not None:
        return _CACHE
    R = rt()
    n = R.bn256_order()
    rnd = random.Random(20240611)
    G = R.g1_generator()
    messages = [R.g1_base_mul(rnd.randrange(1, n)) for _ in range(12)]
    sks = [rnd.randrange(1, n) for _ in range(8)]
    keys = [R.g1_base_mul(s) for s in sks]
    out: list[Case] = []
    scalars: list = []

    def sign(mi: int, ki: int) -> bytes:
        return R.schnorr_sign(messages[mi], be32(sks[ki]), rnd.randbytes(32))

    def sign_with_nonce(mi: int, sk: int, v: int):
        c, _ = challenge(R.g1_base_mul(v), messages[mi])
        return c, (v - sk * c) % n

    # ---- ordinary
    ordinary = []
    for i in range(64):
        mi, ki = i % len(messages), i % len(keys)
        sg = sign(mi, ki)
        ordinary.append((mi, ki, sg))
        out.append(Case(f"ordinary-{i}", mi, ki, sg, 0))

    # ---- chosen r, each under a key of its own
    def chosen_r(name: str, r: int, mi: int):
        while True:
            v = rnd.randrange(1, n)
            c, _ = challenge(R.g1_base_mul(v), messages[mi])
            sk = (v - r) * pow(c, -1, n) % n
            if sk:
                break
        keys.append(R.g1_base_mul(sk))
        ki = len(keys) - 1
        out.append(Case(name, mi, ki, be32(c) + be32(r), 0))
        scalars.append((r, c, ki))

    edge_r = [("r=1", 1), ("r=n-1", n - 1), ("r=0x80..", int.from_bytes(b"\x80" * 32, "big")),
              ("r=0x81..", int.from_bytes(b"\x81" * 32, "big")), ("r=2^8-1", 2 ** 8 - 1), ("r=2^64-1", 2 ** 64 - 1),
              ("r=2^255-1", 2 ** 255 - 1)]
    for i, (name, r) in enumerate(edge_r):
        chosen_r(name, r, i % len(messages))
    # the window-32 carry: top byte above 0x80 (0x81 .. 0x8f)
    for i in range(6):
        top = 0x81 + (i * 3) % 15
        while True:
            r = (top << 248) | rnd.getrandbits(248)
            if r < n:
                break
        chosen_r(f"r-top-{top:#x}", r, (i + 3) % len(messages))
    for i in range(6):
        mi, ki = (i + 5) % len(messages), i % 8
        while True:
            c, r = sign_with_nonce(mi, sks[ki], rnd.randrange(1, n))
            if (c >> 248) > 0x80:
                break
        out.append(Case(f"c-top-{c >> 248:#x}", mi, ki, be32(c) + be32(r), 0))
        scalars.append((r, c, ki))

    # ---- degenerate points
    keys.append(G)                      # sk = 1: r G + c G with r == c runs the doubling branch of the last addition
    kg = len(keys) - 1
    for k in (1, 2, 77):
        out.append(Case(f"key=G r=c={k}", 0, kg, be32(k) + be32(k), 2))
        scalars.append((k, k, kg))
    for i in range(2):                  # forged r = -sk c: T is the point at infinity
        c = rnd.randrange(1, n)
        r = (-sks[i] * c) % n
        out.append(Case(f"T=infinity-{i}", i, i, be32(c) + be32(r), 2))
        scalars.append((r, c, i))
    keys.append(R.g1_infinity())        # sk = 0: c PK vanishes, (c, r) = (H(v G, m), v) is valid
    kinf = len(keys) - 1
    for i in range(2):
        v = rnd.randrange(1, n)
        c, _ = challenge(R.g1_base_mul(v), messages[i])
        out.append(Case(f"key=infinity-{i}", i, kinf, be32(c) + be32(v), 0))
        scalars.append((v, c, kinf))
    out.append(Case("key=infinity-wrong", 2, kinf, ordinary[2][2], 2))

    # ---- invalid: bit flips, the wrong key
    def flip(b: bytes, bit: int) -> bytes:
        a = bytearray(b)
        a[bit >> 3] ^= 1 << (bit & 7)
        return bytes(a)

    for i in range(10):
        mi, ki, sg = ordinary[i]
        bit = rnd.randrange(8, 256)     # (not the top byte: c stays below n)
        out.append(Case(f"flip-c-{i}", mi, ki, flip(sg, bit), 2))
        out.append(Case(f"flip-r-{i}", mi, ki, flip(sg, 256 + bit), 2))
        messages.append(flip(messages[mi], rnd.randrange(512)))
        out.append(Case(f"flip-msg-{i}", len(messages) - 1, ki, sg, 2))
        out.append(Case(f"wrong-key-{i}", mi, (ki + 1 + i % 7) % 8, sg, 2))

    # ---- invalid: range
    mi, ki, sg = ordinary[0]
    c0, r0 = sg[:32], sg[32:]
    out.append(Case("c=n", mi, ki, be32(n) + r0, 1))
    out.append(Case("r=n", mi, ki, c0 + be32(n), 1))
    out.append(Case("c=2^256-1", mi, ki, b"\xff" * 32 + r0, 1))
    out.append(Case("c=0", mi, ki, bytes(32) + r0, 2))

    # ---- invalid: indices (nmsg and nkeys are the final counts: appended last)
    nk, nm = len(keys), len(messages)
    out.append(Case("key_idx=-1", mi, -1, sg, 4))
    out.append(Case("key_idx=nkeys", mi, nk, sg, 4))
    out.append(Case("msg_idx=nmsg", nm, ki, sg, 4))
    out.append(Case("c=n and key_idx=nkeys", mi, nk, be32(n) + r0, 1))   # the range check comes first

    _CACHE = {"keys": keys, "messages": messages, "cases": out, "scalars": scalars, "order": n}
    return _CACHE


def host_status(case: Case, keys, messages):
    """The host verifier's verdict as a status (0 / 1 / 2), None for an index out of range."""
    R = rt()
    n = R.bn256_order()
    c, r = int.from_bytes(case.sig[:32], "big"), int.from_bytes(case.sig[32:], "big")
    if not (0 <= case.key_idx < len(keys) and 0 <= case.msg_idx < len(messages)):
        return 1 if (c >= n or r >= n) else None
    ok = R.schnorr_verify(messages[case.msg_idx], keys[case.key_idx], case.sig)
    if ok:
        return 0
    return 1 if (c >= n or r >= n) else 2
