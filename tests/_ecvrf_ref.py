"""An independent ECVRF-EDWARDS25519-SHA512-TAI (RFC 9381) prover in plain Python: big integers and hashlib
only, nothing of biscotti_amd.  The tests of the host runtime (vrf.cpp, vrf_ifma.cpp) and of the device prover
(kernels/vrf.hip) compare against it.

It takes raw key material -- the secret scalar x as an integer (any 0 <= x < 2^255, clamped or not), the
nonce prefix and the encoded public key -- so crafted scalars can be proved, which a seed-based prover cannot do.
Points are extended coordinates (X, Y, Z, T) with x = X/Z, y = Y/Z, xy = T/Z; one inversion per encoding.
Scalar multiplication is plain double-and-add over the scalar's bits (no recoding, no tables of the point),
so it shares no algorithm with the kernels it checks.
"""
import hashlib

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRTM1 = pow(2, (P - 1) // 4, P)
SUITE = b"\x03"
IDENTITY = (0, 1, 1, 0)


def _sha512(*parts: bytes) -> bytes:
    return hashlib.sha512(b"".join(parts)).digest()


def add(p, q):
    """add-2008-hwcd-3 (a = -1): complete, so it also doubles and takes the identity."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def dbl(p):
    """dbl-2008-hwcd (a = -1)."""
    x1, y1, z1, _ = p
    a = x1 * x1 % P
    b = y1 * y1 % P
    c = 2 * z1 * z1 % P
    e = ((x1 + y1) * (x1 + y1) - a - b) % P
    g = b - a
    f = g - c
    h = -a - b
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k: int, p):
    """k * p for any integer k >= 0, most significant bit first."""
    assert k >= 0
    r = IDENTITY
    for i in range(k.bit_length() - 1, -1, -1):
        r = dbl(r)
        if (k >> i) & 1:
            r = add(r, p)
    return r


def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def enc(p) -> bytes:
    x, y = affine(p)
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(s: bytes):
    """RFC 8032 5.1.3: the point of a 32-byte string, or None (non-canonical y, no square root, x = 0 with
    the sign bit set)."""
    y = int.from_bytes(s, "little")
    sign = y >> 255
    y &= (1 << 255) - 1
    if y >= P:
        return None
    u = (y * y - 1) % P
    v = (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    vx2 = v * x * x % P
    if vx2 != u:
        if vx2 != (P - u) % P:
            return None
        x = x * SQRTM1 % P
    if x == 0 and sign:
        return None
    if (x & 1) != sign:
        x = P - x
    return (x, y, 1, x * y % P)


_BY = 4 * pow(5, P - 2, P) % P
B = decode(_BY.to_bytes(32, "little"))   # the base point: y = 4/5, x even
_B_DOUBLES = []


def mul_base(k: int):
    """k * B over the stored doublings of B (adds only)."""
    assert k >= 0
    while len(_B_DOUBLES) < max(k.bit_length(), 1):
        _B_DOUBLES.append(dbl(_B_DOUBLES[-1]) if _B_DOUBLES else B)
    r = IDENTITY
    for i in range(k.bit_length()):
        if (k >> i) & 1:
            r = add(r, _B_DOUBLES[i])
    return r


def key_from_seed(seed: bytes):
    """RFC 8032 key expansion: (x, prefix, pk) of a 32-byte seed."""
    h = bytearray(_sha512(seed))
    h[0] &= 248
    h[31] &= 127
    h[31] |= 64
    x = int.from_bytes(h[:32], "little")
    return x, bytes(h[32:]), enc(mul_base(x))


def _try(pk: bytes, alpha: bytes, ctr: int):
    return decode(_sha512(SUITE, b"\x01", pk, alpha, bytes([ctr, 0]))[:32])


def first_counter(pk: bytes, alpha: bytes) -> int:
    """The smallest try-and-increment counter whose hash decodes to a point (the one the RFC takes)."""
    for ctr in range(256):
        if _try(pk, alpha, ctr) is not None:
            return ctr
    raise ValueError("no counter decodes")


def encode_to_curve(pk: bytes, alpha: bytes):
    """(H, ctr): H = 8 * (the first decoding candidate), and its counter."""
    ctr = first_counter(pk, alpha)
    return mul(8, _try(pk, alpha, ctr)), ctr


def prove(x: int, prefix: bytes, pk: bytes, alpha: bytes):
    """(pi, beta, ctr): the 80-byte proof Gamma || c || s, the 64-byte output, and the counter of H."""
    assert 0 <= x < 2 ** 255 and len(prefix) == 32 and len(pk) == 32
    h, ctr = encode_to_curve(pk, alpha)
    hstr = enc(h)
    gamma = mul(x, h)
    k = int.from_bytes(_sha512(prefix, hstr), "little") % L
    gstr = enc(gamma)
    c = _sha512(SUITE, b"\x02", pk, hstr, gstr, enc(mul_base(k)), enc(mul(k, h)), b"\x00")[:16]
    s = (k + int.from_bytes(c, "little") * x) % L
    beta = _sha512(SUITE, b"\x03", enc(mul(8, gamma)), b"\x00")
    return gstr + c + s.to_bytes(32, "little"), beta, ctr


def prove_seed(seed: bytes, alpha: bytes):
    return prove(*key_from_seed(seed), alpha)
