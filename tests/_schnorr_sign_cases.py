"""The case set of the Schnorr signer tests: the host's signature rebuilt with plain Python integers over the
runtime's bindings (blake2xb, g1_base_mul), so that the nonce, the challenge and their draw counts are known.

    entropy = base[key] || le32(nonce id);  v = first candidate of blake2xb(entropy, no message) in (0, n)
    T = v G;  c = first candidate of blake2xb(marshal(T), message) in (0, n);  r = v - sk c mod n;  sig = c || r

Ten keys (eight ordinary ones, sk = 1, sk = n - 1), the nonce ids 0, 1, 0x7fffffff, 0x80000000 and 0xffffffff under
every key, items sharing a message, and items found by trying nonce ids whose nonce or challenge needs three draws
or more.  No item may need more than DRAWS draws on either XOF (status 3 must not occur): test_schnorr_sign_cpu
checks it with the host alone.  Built once per process (cases()), never modified.
"""
from __future__ import annotations

import random
from typing import NamedTuple

from biscotti_amd.native import rt

DRAWS = 32
EDGE_IDS = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)


class Item(NamedTuple):
    msg_idx: int
    key_idx: int
    nonce_id: int
    v: int        # the nonce
    vdraws: int   # candidates the nonce needed
    cdraws: int   # candidates the challenge needed
    sig: bytes    # the integer model's 64 bytes


def be32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def entropy(base: bytes, nonce_id: int) -> bytes:
    return bytes(base) + (int(nonce_id) & 0xffffffff).to_bytes(4, "little")


def first_candidate(key: bytes, msg: bytes, limit: int = 64):
    """pick_scalar_from_xof over blake2xb(key, msg): (scalar, candidates drawn)."""
    R = rt()
    n = R.bn256_order()
    stream = R.blake2xb(key, msg, 32 * limit)
    for j in range(limit):
        v = int.from_bytes(stream[32 * j:32 * j + 32], "big")
        if 0 < v < n:
            return v, j + 1
    raise AssertionError("no candidate in %d draws" % limit)


def sign_model(msg: bytes, sk: int, ent: bytes):
    """(signature, nonce, nonce draws, challenge draws) with Python integers."""
    R = rt()
    n = R.bn256_order()
    v, vd = first_candidate(ent, b"")
    c, cd = first_candidate(R.g1_base_mul(v), msg)
    return be32(c) + be32((v - sk * c) % n), v, vd, cd


_CACHE = None


def cases():
    """dict: sks (ints), bases (32 bytes each; key index = position), messages (64 bytes each), items [Item],
    order."""
    global _CACHE
    if _CACHE is not None:
        return _CACHE
    R = rt()
    n = R.bn256_order()
    rnd = random.Random(20240923)
    messages = [R.g1_base_mul(rnd.randrange(1, n)) for _ in range(12)]
    sks = [rnd.randrange(1, n) for _ in range(8)] + [1, n - 1]
    bases = [rnd.randbytes(32) for _ in sks]
    items: list[Item] = []

    def add(mi: int, ki: int, nid: int) -> Item:
        sig, v, vd, cd = sign_model(messages[mi], sks[ki], entropy(bases[ki], nid))
        items.append(Item(mi, ki, nid, v, vd, cd, sig))
        return items[-1]

    for ki in range(len(sks)):                 # every edge id under every key, sk = 1 and sk = n - 1 included
        for j, nid in enumerate(EDGE_IDS):
            add((ki + j) % len(messages), ki, nid)
    for ki in range(len(sks)):                 # one message signed by every key (a worker's commitment, its verifiers)
        add(5, ki, 1000 + ki)
    for i in range(12):                        # one key and one nonce id over different messages
        add(i, 3, 77)
    # found by trying nonce ids: a nonce and a challenge that need three draws or more (about 15 % of items each)
    nid = 2000
    while not (any(it.vdraws >= 3 for it in items) and any(it.cdraws >= 3 for it in items)) or len(items) < 90:
        add(nid % len(messages), nid % len(sks), nid)
        nid += 1
        assert nid < 3000, "no multi-draw item found"
    _CACHE = {"sks": sks, "bases": bases, "messages": messages, "items": items, "order": n}
    return _CACHE
