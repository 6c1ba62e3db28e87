"""An ECVRF-EDWARDS25519-SHA512-TAI (RFC 9381) verifier in plain Python on top of _ecvrf_ref.py, and the tamper
set the verifier tests share.  The checks and their order are those of runtime/vrf.cpp::vrf_verify; the status
codes are those of the device verifier (kernels/vrf.hip, k_vrf_verify):

  0 valid | 1 the public key does not decode | 2 Gamma does not decode | 3 s >= L | 4 the challenge differs
  5 valid, but proof_to_hash differs from the expected output supplied for it

test_vrf_verify_ref.py pins it to the RFC's example vector and to the host runtime before a GPU is involved.
"""
import hashlib

import _ecvrf_ref as E
import test_vrf_edges as V

ZERO_BETA = bytes(64)

_h_cache: dict = {}


def neg(p):
    return ((E.P - p[0]) % E.P, p[1], p[2], (E.P - p[3]) % E.P)


def _h(pk: bytes, alpha: bytes):
    h = _h_cache.get((pk, alpha))
    if h is None:
        h = _h_cache[(pk, alpha)] = E.encode_to_curve(pk, alpha)[0]
    return h


def verify(pk: bytes, alpha: bytes, pi: bytes, expect: bytes | None = None):
    """(status, beta): beta is the 64-byte output for status 0 and 5, 64 zero bytes otherwise."""
    assert len(pk) == 32 and len(pi) == 80
    y = E.decode(pk)
    if y is None:
        return 1, ZERO_BETA
    gamma = E.decode(pi[:32])
    if gamma is None:
        return 2, ZERO_BETA
    c = int.from_bytes(pi[32:48], "little")
    s = int.from_bytes(pi[48:], "little")
    if s >= E.L:
        return 3, ZERO_BETA
    h = _h(pk, alpha)
    u = E.add(E.mul_base(s), neg(E.mul(c, y)))
    v = E.add(E.mul(s, h), neg(E.mul(c, gamma)))
    c2 = hashlib.sha512(E.SUITE + b"\x02" + pk + E.enc(h) + pi[:32] + E.enc(u) + E.enc(v) + b"\x00").digest()[:16]
    if c2 != pi[32:48]:
        return 4, ZERO_BETA
    beta = hashlib.sha512(E.SUITE + b"\x03" + E.enc(E.mul(8, gamma)) + b"\x00").digest()
    if expect is not None and expect != beta:
        return 5, beta
    return 0, beta


# ------------------------------------------------------------------------------------------- the tamper set
BASE_SEED = V.seed_of(0x07)
BASE_ALPHA = bytes(range(32))
OTHER_SEED = V.seed_of(0x08)
N_FLIPS = 640


def tamper_cases():
    """[(name, pk, alpha, pi)]: the 640 single-bit flips of one proof first (case i flips bit i % 8 of byte
    i // 8), then the named cases."""
    _, _, pk = E.key_from_seed(BASE_SEED)
    pi = E.prove_seed(BASE_SEED, BASE_ALPHA)[0]
    out = []
    for bit in range(N_FLIPS):
        b = bytearray(pi)
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append((f"flip-{bit}", pk, BASE_ALPHA, bytes(b)))
    s = int.from_bytes(pi[48:], "little")
    assert s + E.L < 2 ** 256
    p1 = (E.P + 1).to_bytes(32, "little")
    out.append(("s+L", pk, BASE_ALPHA, pi[:48] + (s + E.L).to_bytes(32, "little")))
    out.append(("wrong-message", pk, bytes(32), pi))
    out.append(("wrong-key", E.key_from_seed(OTHER_SEED)[2], BASE_ALPHA, pi))
    out.append(("pk-P+1", p1, BASE_ALPHA, pi))
    out.append(("gamma-P+1", pk, BASE_ALPHA, p1 + pi[32:]))
    for name, x in V.CRAFTED_X.items():
        row = V.crafted_row(x)
        for j, alpha in enumerate(V.CRAFTED_ALPHAS):
            out.append((f"crafted-{name}-{j}", row[2], alpha, E.prove(*row, alpha)[0]))
    out.append(("untampered", pk, BASE_ALPHA, pi))
    return out


def rfc_case():
    """The RFC 9381 example vector (an empty message, so a launch of its own on the device)."""
    return "rfc", E.key_from_seed(V.RFC_SEED)[2], b"", bytes.fromhex(V.RFC_PI)


_cases = None
_ref = None


def cases():
    global _cases
    if _cases is None:
        _cases = tamper_cases()
    return _cases


def reference():
    """[(status, beta)] of verify over cases(), computed once per session."""
    global _ref
    if _ref is None:
        _ref = [verify(pk, alpha, pi) for _, pk, alpha, pi in cases()]
    return _ref
