"""ECVRF edges the random tests never reach: a hash-to-curve counter of 12 and more (the device prover's second
pass of 12 counters, the IFMA batch's late lanes), scalars whose signed radix-16 recoding carries through every
digit or ends in +8, and message lengths around the SHA-512 block edges.

This module pins the plain-Python reference (_ecvrf_ref.py) to RFC 9381 and to the host runtime, holds the
committed inputs (found by scanning with the reference; every counter is re-derived here, so they cannot go
stale), and runs them through every host path.  tests/test_gpu_vrf.py runs the same inputs on the device.

Not covered, because no input can be steered there: a hash whose y is non-canonical (>= p, probability about
2^-250 per try) and a (key, message) pair with no decoding counter at all (2^-256).
"""
import hashlib

import pytest

import _ecvrf_ref as E
from biscotti_amd.native import rt

RFC_SEED = bytes.fromhex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60")
RFC_PI = ("8657106690b5526245a92b003bb079ccd1a92130477671f6fc01ad16f26f723f26f8a57ccaed74ee1b190b"
          "ed1f479d9727d2d0f9b005a6e456a35d4fb0daab1268a1b0db10836d9826a528ca76567805")
RFC_BETA = ("90cf1df3b703cce59e2a35b925d411164068269d7b2d29f3301c03dd757876ff66b71dda49d2de59d0345"
            "0451af026798e8f81cd2e333de5cdf4f3e140fdd8ae")


def seed_of(b: int) -> bytes:
    return bytes([b]) * 32


def alpha_of(i: int) -> bytes:
    return i.to_bytes(32, "little")


def det_bytes(tag: str, n: int) -> bytes:
    """n reproducible bytes."""
    return hashlib.shake_256(tag.encode()).digest(n)


# (seed byte, alpha number, first decoding counter): seed = seed_of(b), alpha = alpha_of(i).  Found by scanning
# alpha numbers 0..23999 for the seeds 01.., 04.. with _ecvrf_ref.first_counter.
LOW_COUNTER = [(2, 0, 0), (1, 0, 1), (4, 0, 2), (1, 9, 3), (2, 1, 4), (1, 4, 5), (2, 23, 6), (4, 47, 7),
               (3, 264, 8), (2, 151, 9), (4, 667, 10), (4, 1863, 11)]
HIGH_COUNTER = [(3, 987, 15), (4, 2194, 12), (2, 3371, 12), (2, 3518, 13), (1, 4004, 15), (1, 4907, 14),
                (1, 5029, 13), (2, 7013, 12), (1, 7349, 14), (1, 8166, 17), (4, 8833, 13), (4, 9036, 13),
                (1, 10841, 12), (1, 11804, 12), (1, 13670, 12), (1, 14521, 13), (3, 14951, 12), (2, 17672, 13),
                (3, 20359, 15), (3, 20470, 15), (1, 20782, 14), (4, 21040, 12), (4, 22106, 12), (2, 23647, 12)]
# one alpha for eight keys (one IFMA batch): exactly one lane needs 12 or more attempts, the others 0..2
IFMA_SEEDS = [seed_of(0x10 + j) for j in range(8)]
IFMA_ALPHAS = [(1227, [0, 0, 0, 2, 0, 0, 0, 13]), (2188, [1, 0, 1, 0, 0, 0, 12, 1]),
               (3865, [1, 12, 2, 0, 0, 0, 0, 0]), (5155, [0, 1, 2, 0, 12, 2, 1, 0]),
               (5814, [13, 0, 0, 0, 1, 2, 0, 0]), (6113, [2, 0, 12, 0, 1, 1, 2, 0]),
               (14853, [0, 2, 0, 14, 0, 0, 1, 0]), (15046, [2, 0, 2, 1, 0, 13, 2, 2])]

# ---- crafted secret scalars (the device kernel's contract is x < 2^255, not "clamped")
CRAFTED_PREFIX = bytes(range(0xA0, 0xC0))
CRAFTED_X = {
    "2^255-8": 2 ** 255 - 8,                    # the largest clamped scalar: a carry through all 64 digits, top +8
    "2^254": 2 ** 254,                          # a single non-zero digit
    "nibbles-7": int("7" * 64, 16),             # no carries
    "nibbles-8": int("0" + "8" * 63, 16),       # -8, then -7 with a carry out of every digit
    "digits--8": int("0" + "7" * 62 + "8", 16),   # digit -8 in every position below the top
    "8": 8,
    "0": 0,                                     # Gamma is the identity
    "L": E.L,                                   # Gamma is the identity, s = k
    "L-1": E.L - 1,                             # Gamma = -H
    "L+1": E.L + 1,                             # Gamma = H
    "2^252": 2 ** 252,
    "2^252-1": 2 ** 252 - 1,
}
CRAFTED_ALPHAS = [det_bytes("crafted alpha 0", 32), det_bytes("crafted alpha 1", 32)]

# 36 + n bytes are hashed: the 0x80 and the length still fit the block up to n = 75; for n = 76..90 (and 204..218)
# the padding spills into a block of its own; at 91 the 0x80 fills the block; at 92 the message does
ALPHA_LENS = [0, 1, 75, 76, 90, 91, 92, 93, 203, 204, 220, 1024]
LEN_SEEDS = [seed_of(0x31), seed_of(0x32), seed_of(0x33)]
LEN_KEY_IDX = [2, 0, 1, 2, 0]
LEN_ALPHA_IDX = [1, 0, 1, 0, 1]

POOL_SEEDS = [seed_of(0x40 + i) for i in range(33)]
POOL_ALPHAS = [det_bytes(f"pool alpha {i}", 32) for i in range(4)]
BATCH_NS = [1, 15, 16, 17, 33]


def signed_digits(x: int):
    """The signed radix-16 digits (least significant first) of x < 2^255: every digit in [-8, 8) but the top."""
    e = [(x >> (4 * i)) & 15 for i in range(64)]
    carry = 0
    for i in range(63):
        e[i] += carry
        carry = (e[i] + 8) >> 4
        e[i] -= carry << 4
    e[63] += carry
    assert sum(d << (4 * i) for i, d in enumerate(e)) == x
    return e


def crafted_row(x: int):
    """(x, prefix, pk) with pk = x * B."""
    return x, CRAFTED_PREFIX, E.enc(E.mul_base(x))


def row_bytes(x: int, prefix: bytes, pk: bytes) -> bytes:
    """The device prover's 96-byte key row."""
    return x.to_bytes(32, "little") + prefix + pk


def len_alphas(n: int):
    return [det_bytes(f"alpha {n} a", n), det_bytes(f"alpha {n} b", n)]


# ---- the device tests' inputs, as lists of (seed, alpha)
def _pair(entry):
    return seed_of(entry[0]), alpha_of(entry[1])


def _by_counter():
    m = {}
    for e in LOW_COUNTER + HIGH_COUNTER:
        m.setdefault(e[2], []).append(e)
    return m


# lane p of the mixed workgroup has this first counter; the lanes at 12 and more are 1, 4, 6, 8, 11 and 13
MIX_COUNTERS = [0, 12, 1, 11, 13, 0, 15, 1, 17, 11, 0, 14, 1, 12, 0, 11]


def inputs_counter_mix():
    m, used, out = _by_counter(), {}, []
    for c in MIX_COUNTERS:
        k = used.get(c, 0)
        used[c] = k + 1
        out.append(_pair(m[c][k % len(m[c])]))
    return out


def inputs_counter_high():
    """16 proofs, every one with a first counter of 12 or more (the 17 among them)."""
    return [_pair(e) for e in HIGH_COUNTER[:16]]


def inputs_counter_slots():
    """12 workgroups of 16: lane p of workgroup g has first counter (g + p) % 12, so lane 0 of the workgroups
    runs through every publishing slot 0..11 (and so does every other lane)."""
    return [_pair(LOW_COUNTER[(g + p) % 12]) for g in range(12) for p in range(16)]


def inputs_lens():
    return [(LEN_SEEDS[k], len_alphas(n)[a]) for n in ALPHA_LENS for k, a in zip(LEN_KEY_IDX, LEN_ALPHA_IDX)]


def inputs_batch():
    return [(POOL_SEEDS[i], POOL_ALPHAS[i % 2]) for i in range(33)]


# the wrapper tests: rounds as (slice of POOL_SEEDS, index into POOL_ALPHAS)
WRAP_ONE = [(slice(0, 21), 0)]
WRAP_TWO = [(slice(0, 20), 1), (slice(10, 27), 2)]
WRAP_THREE = [(slice(3, 10), 3), (slice(0, 18), 0), (slice(28, 33), 1)]
WRAP_THREE_SMALL = [(slice(30, 33), 2), (slice(5, 7), 3), (slice(12, 16), 0)]
WRAP_ROWS = [(slice(8, 19), 3)]
PROVE_FIRST = [(0, 0), (1, 1), (0, 0), (2, 2), (1, 1), (0, 1), (3, 0), (0, 2)]   # (seed, alpha): repeats, a b a c b
PROVE_SECOND = [(20, 1), (0, 0), (21, 3), (1, 1), (20, 0), (3, 3)]   # new seeds after the key table's upload


def inputs_wrapper():
    out = []
    for rounds in (WRAP_ONE, WRAP_TWO, WRAP_THREE, WRAP_THREE_SMALL, WRAP_ROWS):
        for sl, a in rounds:
            out += [(s, POOL_ALPHAS[a]) for s in POOL_SEEDS[sl]]
    out += [(POOL_SEEDS[s], POOL_ALPHAS[a]) for s, a in PROVE_FIRST + PROVE_SECOND]
    return out


def device_seed_inputs():
    """Every (seed, alpha) pair the device tests prove from a seed, without repeats."""
    allp = (inputs_counter_mix() + inputs_counter_high() + inputs_counter_slots() + inputs_lens() + inputs_batch()
            + inputs_wrapper())
    return list(dict.fromkeys(allp))


_expected: dict = {}


def expected(seed: bytes, alpha: bytes):
    """(pi, beta) of the reference, computed once per pair and shared by the tests."""
    r = _expected.get((seed, alpha))
    if r is None:
        r = _expected[(seed, alpha)] = E.prove_seed(seed, alpha)[:2]
    return r


# ------------------------------------------------------------------------------------------- the reference
def test_reference_reproduces_rfc9381_vector():
    pi, beta, ctr = E.prove_seed(RFC_SEED, b"")
    assert pi.hex() == RFC_PI and beta.hex() == RFC_BETA
    R = rt()
    assert R.vrf_prove(RFC_SEED, b"") == (beta, pi)
    assert E.key_from_seed(RFC_SEED)[2] == R.vrf_public_key(RFC_SEED)


def test_reference_point_arithmetic():
    assert E.enc(E.mul_base(E.L)) == E.enc(E.IDENTITY) == (1).to_bytes(32, "little")
    assert E.enc(E.mul(E.L - 1, E.B)) == E.enc((E.P - E.B[0], E.B[1], 1, E.P - E.B[3]))
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
    assert E.enc(E.mul(k, E.B)) == E.enc(E.mul_base(k))
    assert E.enc(E.add(E.mul_base(k), E.mul_base(7))) == E.enc(E.mul_base(k + 7))
    assert E.enc(E.dbl(E.mul_base(k))) == E.enc(E.mul_base(2 * k))
    assert E.decode(E.enc(E.mul_base(k)))[:2] == E.affine(E.mul_base(k))
    assert E.decode((E.P + 1).to_bytes(32, "little")) is None   # non-canonical y
    assert E.decode(((1 << 255) | 1).to_bytes(32, "little")) is None   # x = 0 with the sign bit


def test_committed_counters_are_rederived():
    assert sorted(c for _, _, c in LOW_COUNTER) == list(range(12))
    assert len(HIGH_COUNTER) >= 16 and all(c >= 12 for _, _, c in HIGH_COUNTER)
    assert any(c >= 13 for _, _, c in HIGH_COUNTER)
    for b, i, c in LOW_COUNTER + HIGH_COUNTER:
        assert E.first_counter(E.key_from_seed(seed_of(b))[2], alpha_of(i)) == c, (b, i)
    pks = [E.key_from_seed(s)[2] for s in IFMA_SEEDS]
    for i, ctrs in IFMA_ALPHAS:
        assert [E.first_counter(pk, alpha_of(i)) for pk in pks] == ctrs, i
        assert max(ctrs) >= 12 and sorted(ctrs)[-2] <= 2
    assert len({ctrs.index(max(ctrs)) for _, ctrs in IFMA_ALPHAS}) == 8   # the late lane is each lane once
    # the mixed workgroup really is what its test says
    assert [E.first_counter(E.key_from_seed(s)[2], a) for s, a in inputs_counter_mix()] == MIX_COUNTERS
    assert {0, 1, 11, 12} <= set(MIX_COUNTERS) and max(MIX_COUNTERS) >= 13


def test_reference_equals_host_on_every_device_input():
    R = rt()
    pairs = device_seed_inputs()
    for s in dict.fromkeys(s for s, _ in pairs):
        assert row_bytes(*E.key_from_seed(s)) == R.vrf_key_material(s)
    for s, a in pairs:
        pi, beta = expected(s, a)
        assert R.vrf_prove(s, a) == (beta, pi), (s[:1].hex(), len(a))


def test_crafted_scalars_recode_as_claimed_and_verify():
    d = {name: signed_digits(x) for name, x in CRAFTED_X.items()}
    assert d["2^255-8"] == [-8] + [0] * 62 + [8]
    assert d["2^254"] == [0] * 63 + [4]
    assert d["nibbles-7"] == [7] * 64
    assert d["nibbles-8"] == [-8] + [-7] * 62 + [1]
    assert d["digits--8"] == [-8] * 63 + [1]
    assert d["8"] == [-8, 1] + [0] * 62
    R = rt()
    for name, x in CRAFTED_X.items():
        assert 0 <= x < 2 ** 255
        row = crafted_row(x)
        for alpha in CRAFTED_ALPHAS:
            pi, beta, _ = E.prove(*row, alpha)
            gamma = E.decode(pi[:32])
            if x % E.L == 0:
                assert pi[:32] == E.enc(E.IDENTITY), name
            else:
                assert R.vrf_verify(row[2], alpha, pi) == beta, name
            h, _ = E.encode_to_curve(row[2], alpha)
            if name == "L+1":
                assert pi[:32] == E.enc(h)
            if name == "L-1":
                assert E.enc(E.add(gamma, h)) == E.enc(E.IDENTITY)


# ------------------------------------------------------------------------------------------- the host paths
def _which():
    path = "AVX-512 IFMA batch" if rt().vrf_beta_batch_supported() else "scalar fallback (no IFMA on this CPU)"
    print(f"vrf batch path under test: {path}")
    return path


def test_host_batch_paths_with_one_late_lane():
    """One alpha for eight keys, exactly one of which needs 12 to 14 attempts while the others need 0..2: the
    IFMA batch keeps hashing that lane alone.  Every host path gives the scalar path's and the reference's bytes."""
    R = rt()
    _which()
    for i, ctrs in IFMA_ALPHAS:
        alpha = alpha_of(i)
        scalar = [R.vrf_prove(s, alpha) for s in IFMA_SEEDS]
        late = ctrs.index(max(ctrs))
        for lane in {late, (late + 1) % 8}:   # the late lane and a neighbour against the reference
            pi, beta, ctr = E.prove_seed(IFMA_SEEDS[lane], alpha)
            assert ctr == ctrs[lane] and scalar[lane] == (beta, pi)
        betas = [b for b, _ in scalar]
        assert R.vrf_beta_batch(IFMA_SEEDS, alpha) == betas, i
        assert R.vrf_prove_batch_ifma(IFMA_SEEDS, alpha) == scalar, i
        assert R.vrf_prove_batch_async(IFMA_SEEDS, alpha, 2, None, True).betas() == betas, i
        assert R.vrf_proofs_async(IFMA_SEEDS, alpha, 2).result() == scalar, i
        # a partial batch whose last lane is the late one, and the late lane alone
        assert R.vrf_beta_batch(IFMA_SEEDS[:late + 1], alpha) == betas[:late + 1], i
        assert R.vrf_prove_batch_ifma(IFMA_SEEDS[late:late + 1], alpha) == scalar[late:late + 1], i


def test_host_batch_paths_over_high_counter_pairs():
    """Every committed pair with a first counter of 12..17, batched with eleven other keys over the same alpha."""
    R = rt()
    _which()
    for b, i, c in HIGH_COUNTER:
        alpha = alpha_of(i)
        seeds = IFMA_SEEDS[:5] + [seed_of(b)] + IFMA_SEEDS[5:] + [seed_of(k) for k in (1, 2, 3, 4) if k != b]
        scalar = [R.vrf_prove(s, alpha) for s in seeds]
        pi, beta, ctr = E.prove_seed(seed_of(b), alpha)
        assert ctr == c and scalar[5] == (beta, pi)
        betas = [x for x, _ in scalar]
        assert R.vrf_beta_batch(seeds, alpha) == betas, (b, i)
        assert R.vrf_prove_batch_ifma(seeds, alpha) == scalar, (b, i)
        assert R.vrf_prove_batch_async(seeds, alpha, 2, None, True).betas() == betas, (b, i)
        assert R.vrf_proofs_async(seeds, alpha, 2).result() == scalar, (b, i)


@pytest.mark.parametrize("n", ALPHA_LENS)
def test_host_batch_paths_at_block_edge_lengths(n):
    R = rt()
    for alpha in len_alphas(n):
        scalar = [R.vrf_prove(s, alpha) for s in IFMA_SEEDS]
        assert R.vrf_prove_batch_ifma(IFMA_SEEDS, alpha) == scalar
        assert R.vrf_beta_batch(IFMA_SEEDS, alpha) == [b for b, _ in scalar]
        pi, beta, _ = E.prove_seed(IFMA_SEEDS[0], alpha)
        assert scalar[0] == (beta, pi)
