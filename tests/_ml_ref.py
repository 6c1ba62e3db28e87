"""References and case lists of the learning-kernel edge tests: plain numpy fp64 and Python integers.

Nothing here runs torch, and of the code under test only the two definitions of the random streams are used:
K.minibatch_indices (which rows a peer draws) and K.philox4x32 (the counter-based generator).  Every case list is
built once per process and never modified; tests/test_ml_ref_cpu.py vets each case against the project's CPU paths
before tests/test_gpu_ml_edges.py takes it to the kernels.
"""
from __future__ import annotations

import zlib
from fractions import Fraction
from functools import lru_cache
from math import lcm
from typing import NamedTuple

import numpy as np

from biscotti_amd.ops import ml as K

M32 = 0xFFFFFFFF
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
QSCALE = 1e4


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------- softmax step
def softmax_step_ref(X, y, off, ntrain, pid, W, d_in, d_out, B, seed, iteration, max_norm=100.0, lo=-1):
    """fp64 local step of every peer: (delta [P, nparam], loss [P]).  Mean cross-entropy over Bq = min(B, n) rows
    of (x - 0.5) * 2, gradient / Bq, clipped by max_norm / (norm + 1e-6), delta = -grad."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    Wt, bt = W[: d_out * d_in].reshape(d_out, d_in), W[d_out * d_in:]
    P = len(pid)
    delta = np.zeros((P, d_out * d_in + d_out))
    loss = np.zeros(P)
    for p in range(P):
        li = int(pid[p]) - lo if lo >= 0 else p
        n, o = int(ntrain[li]), int(off[li])
        idx = K.minibatch_indices(int(pid[p]), iteration, n, B, seed)
        Bq = min(B, n)
        assert len(idx) == Bq
        rows = [o + i for i in idx]
        xb = (X[rows] - 0.5) * 2.0
        lab = np.asarray(y)[rows].astype(np.int64)
        logits = xb @ Wt.T + bt
        m = logits.max(1, keepdims=True)
        e = np.exp(logits - m)
        se = e.sum(1, keepdims=True)
        r = np.arange(Bq)
        loss[p] = ((m[:, 0] + np.log(se[:, 0])) - logits[r, lab]).mean()
        g = e / se
        g[r, lab] -= 1.0
        g /= Bq
        flat = np.concatenate([(g.T @ xb).reshape(-1), g.sum(0)])
        coef = max_norm / (np.sqrt((flat * flat).sum()) + 1e-6)
        if coef < 1:
            flat = flat * coef
        delta[p] = -flat
    return delta, loss


class SmCase(NamedTuple):
    name: str
    X: np.ndarray      # fp32 [Ntot, d_in]
    y: np.ndarray      # int32 [Ntot]
    off: np.ndarray    # int64
    nt: np.ndarray     # int32
    pid: np.ndarray    # int32 [P]
    W: np.ndarray      # fp64 [nparam]
    d_in: int
    d_out: int
    B: int
    seed: int
    it: int
    lo: int

    @property
    def tol(self):
        """test_gpu_ml.py's own: one LDS tile, or K-tiled."""
        return (5e-4, 5e-6) if self.d_in > 1024 else (2e-4, 2e-6)


SM_SEED = 0xC0FFEE1234567890


def _sm(name, ns, B, d_in, d_out, pid=None, seed=SM_SEED, it=5, lo=-1) -> SmCase:
    g = _rng("sm" + name)
    ntot = int(sum(ns))
    X = g.random((ntot, d_in), dtype=np.float32)
    y = g.integers(0, d_out, ntot).astype(np.int32)
    off = (np.cumsum([0] + list(ns))[:-1]).astype(np.int64)
    nt = np.asarray(ns, np.int32)
    pid = np.asarray(pid if pid is not None else [3 + 7 * i for i in range(len(ns))], np.int32)
    W = g.standard_normal(d_out * d_in + d_out) * (0.05 if d_in <= 1024 else 0.01)
    return SmCase(name, X, y, off, nt, pid, W, d_in, d_out, B, seed, it, lo)


@lru_cache(maxsize=None)
def softmax_cases() -> tuple:
    cs = [_sm(f"n{n}_B{B}", [n, n], B, 33, 10) for n, B in [(3, 10), (1, 10), (10, 10), (16, 16), (40, 1), (40, 10)]]
    cs.append(_sm("mixed_n", [3, 16, 40], 10, 33, 10))
    cs += [_sm(f"din{d}", [12, 12], 10, d, 10) for d in (1, 3, 15, 17, 1023, 1024, 1025, 2049)]
    cs += [_sm("dout2", [12, 12], 10, 17, 2), _sm("dout16", [12, 12], 10, 17, 16),
           _sm("dout16_tiled", [12, 12], 10, 1025, 16)]
    cs.append(_sm("pid_max", [12, 12], 10, 17, 10, pid=[2 ** 31 - 1, 0]))
    cs.append(_sm("iter_max", [12, 12], 10, 17, 10, it=2 ** 31 - 1))
    # resident indexing: off / nt cover six local peers, the launch takes four of them out of order, every n < B
    lo = 40
    cs.append(_sm("lo_subset", [3, 5, 7, 2, 9, 4], 10, 33, 10, pid=[lo + 3, lo + 0, lo + 5, lo + 2], lo=lo))
    return tuple(cs)


@lru_cache(maxsize=None)
def softmax_refs() -> dict:
    return {c.name: softmax_step_ref(c.X, c.y, c.off, c.nt, c.pid, c.W, c.d_in, c.d_out, c.B, c.seed, c.it, lo=c.lo)
            for c in softmax_cases()}


def onehot_softmax(n: int, P: int = 8):
    """Minibatch decoding inputs: W = 0, two classes, every label 0, peer p's rows the n x n identity.  Then
    G[s][0] = -1 / (2 Bq) on every drawn row and, with xs = (x - 0.5) * 2 = +1 on the diagonal and -1 off it,
    delta[p][k] = -(2 - Bq) * (-1 / (2 Bq)) = (2 - Bq) / (2 Bq) if row k was drawn and -1/2 if not."""
    X = np.tile(np.eye(n, dtype=np.float32), (P, 1))
    y = np.zeros(P * n, np.int32)
    off = (np.arange(P) * n).astype(np.int64)
    nt = np.full(P, n, np.int32)
    pid = (np.arange(P) * 5 + 1).astype(np.int32)
    W = np.zeros(2 * n + 2)
    return X, y, off, nt, pid, W


def decode_softmax(delta_row: np.ndarray, n: int, B: int) -> set:
    Bq = min(B, n)
    chosen, rest = (2 - Bq) / (2 * Bq), -0.5
    v = np.asarray(delta_row, np.float64)[:n]
    assert np.all((np.abs(v - chosen) < 1e-5) | (np.abs(v - rest) < 1e-5)), v
    return set(np.nonzero(np.abs(v - chosen) < 1e-5)[0].tolist())


# ---------------------------------------------------------------------------- Gaussian draws
def gauss64(a, b):
    """fp64 Box-Muller on the kernels' 24-bit uniforms ((v >> 8) + 0.5) / 2^24."""
    u1 = ((np.asarray(a, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((np.asarray(b, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# ---------------------------------------------------------------------------- logistic step
def logreg_step_ref(X, y, off, nrows, pid, W, B, seed, calls, alpha, lammy, sigma):
    """fp64 logistic step: (v [P, D], residuals per peer).  The gradient is divided by B (not Bq); the noise uses the
    kernel's counters (k, calls % 100, pid, 0xD9) and key words (seed >> 7, seed >> 39)."""
    X, y, W = np.asarray(X, np.float64), np.asarray(y, np.float64), np.asarray(W, np.float64)
    P, D = len(off), X.shape[1]
    out = np.zeros((P, D))
    residuals = []
    for p in range(P):
        n = int(nrows[p])
        idx = K.minibatch_indices(int(pid[p]), int(calls[p]), n, B, seed, tag=0x106)
        rows = [int(off[p]) + i for i in idx]
        xb, yb = X[rows], y[rows]
        t = yb * (xb @ W)
        with np.errstate(over="ignore"):
            res = -yb / np.exp(np.logaddexp(0.0, t))
        residuals.append(res)
        v = -alpha * (xb.T @ res / B + lammy * W)
        if float(sigma[p]) > 0:
            r = K.philox4x32(np.arange(D), int(calls[p]) % 100, int(pid[p]), 0xD9, (seed >> 7) & M32, (seed >> 39) & M32)
            v = v + (-alpha / B) * float(sigma[p]) * np.sqrt(float(B)) * gauss64(r[0], r[1])
        out[p] = v
    return out, residuals


class LrCase(NamedTuple):
    name: str
    X: np.ndarray      # fp64 [Ntot, D]
    y: np.ndarray      # fp64 [Ntot]
    off: np.ndarray
    nrows: np.ndarray
    pid: np.ndarray
    W: np.ndarray
    B: int
    seed: int
    calls: np.ndarray
    alpha: float
    lammy: float
    sigma: np.ndarray


LR_SEED = 0xA5A5A5A5DEADBEEF


def _lr(name, D, n, B, sigma=(0.0, 0.5, 1.0), calls=(1, 100, 205)) -> LrCase:
    g = _rng("lr" + name)
    P = len(sigma)
    X = g.standard_normal((P * n, D))
    y = np.where(g.random(P * n) > 0.5, 1.0, -1.0)
    off = (np.arange(P) * n).astype(np.int64)
    nrows = np.full(P, n, np.int32)
    pid = np.asarray([0, 1, 2 ** 31 - 1][:P], np.int32)
    W = g.standard_normal(D) * 0.1
    return LrCase(name, X, y, off, nrows, pid, W, B, LR_SEED, np.asarray(calls, np.int32), 1e-2, 1e-2,
                  np.asarray(sigma, np.float64))


def saturated_case(lammy: float) -> LrCase:
    """Four rows, all drawn (n = B = 4), X diagonal with +-800.5 and W = 1, so y * z = +-800.5: rows 0 and 3 take
    the t > 0 branch (exp overflows, residual exactly 0), rows 1 and 2 the other (log1p(exp(-800.5)) = 0, residual
    exactly -y).  Column k of the gradient sees row k alone."""
    X = np.diag([800.5, -800.5, 800.5, -800.5])
    y = np.asarray([1.0, 1.0, -1.0, -1.0])
    return LrCase(f"saturated_lammy{lammy}", X, y, np.zeros(1, np.int64), np.asarray([4], np.int32),
                  np.asarray([9], np.int32), np.ones(4), 4, LR_SEED, np.asarray([3], np.int32), 0.0123, lammy,
                  np.zeros(1))


@lru_cache(maxsize=None)
def logreg_cases() -> tuple:
    cs = [_lr(f"D{D}", D, 100, 10) for D in (1, 64, 65, 130)]
    cs += [_lr(f"n{n}_B{B}", 7, n, B) for n, B in [(5, 10), (64, 64), (100, 10)]]
    cs.append(saturated_case(0.01))
    return tuple(cs)


@lru_cache(maxsize=None)
def logreg_refs() -> dict:
    return {c.name: logreg_step_ref(c.X, c.y, c.off, c.nrows, c.pid, c.W, c.B, c.seed, c.calls, c.alpha, c.lammy,
                                    c.sigma) for c in logreg_cases()}


def f32_ulp(v):
    """One fp32 unit in the last place at float32(v)."""
    return np.spacing(np.abs(np.asarray(v, np.float64).astype(np.float32))).astype(np.float64)


def logreg_atol(c: LrCase, ref: np.ndarray) -> np.ndarray:
    """[P, D] bound on |delta - float32(ref)|: one fp32 ulp (the final rounding; the fp64 accumulation error is far
    below it), plus, on rows with noise, the project's 1e-4 bound on a device N(0, 1) draw times the noise factor."""
    noise = 1e-4 * np.abs(c.alpha / c.B * c.sigma * np.sqrt(float(c.B)))
    return f32_ulp(ref) + noise[:, None]


def onehot_logreg(n: int, P: int = 8):
    """Minibatch decoding inputs: W = 0 and X the n x n identity per peer, so every residual is -y / 2 and
    g[k] = -y_k / (2 B) on drawn rows, 0 elsewhere: delta[p][k] = alpha * y_k / (2 B) or 0."""
    g = _rng(f"lr1h{n}")
    X = np.tile(np.eye(n), (P, 1))
    y = np.where(g.random(P * n) > 0.5, 1.0, -1.0)
    off = (np.arange(P) * n).astype(np.int64)
    nrows = np.full(P, n, np.int32)
    pid = (np.arange(P) * 3 + 2).astype(np.int32)
    return X, y, off, nrows, pid, np.zeros(n)


# ---------------------------------------------------------------------------- DP noise
def dp_noise_ref(delta, noisers, scales, seed, iteration):
    """delta + mean over a worker's nn noisers of scale * N(0, 1; noiser, iteration % 100), in fp64."""
    delta = np.asarray(delta, np.float64)
    P, D = delta.shape
    nn = noisers.shape[1] if noisers.ndim == 2 else 0
    acc = np.zeros((P, D))
    for p in range(P):
        for j in range(nn):
            r = K.philox4x32(np.arange(D), iteration % 100, int(noisers[p, j]), 0xA11CE, seed & M32, (seed >> 32) & M32)
            acc[p] += float(scales[p, j]) * gauss64(r[0], r[1])
    return delta + (acc / nn if nn else 0.0)


DP_SEED = 0x9E3779B97F4A7C15
DP_DIMS = (1, 255, 257)


def dp_case(D: int):
    """(delta fp32 [3, D], noisers int32 [3, 2] with ids 0 and 2^31 - 1, scales fp32 [3, 2] with one zero)."""
    g = _rng(f"dp{D}")
    delta = g.standard_normal((3, D)).astype(np.float32)
    noisers = np.asarray([[0, 2 ** 31 - 1], [5, 0], [2 ** 31 - 1, 7]], np.int32)
    scales = np.asarray([[-0.77, 0.31], [0.0, -1.25], [0.5, 0.5]], np.float32)
    return delta, noisers, scales


# ---------------------------------------------------------------------------- recovery
def basis_order(xs, poly: int) -> list:
    """Positions of the poly x-points of smallest (|x|, x)."""
    return sorted(range(len(xs)), key=lambda i: (abs(int(xs[i])), int(xs[i])))[:poly]


@lru_cache(maxsize=None)
def inverse_vandermonde(nodes: tuple):
    """(A, Dn): the inverse of [x_i^k] over the rationals as an integer matrix A over its common denominator Dn."""
    n = len(nodes)
    M = [[Fraction(x) ** k for k in range(n)] for x in nodes]
    inv = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p], inv[c], inv[p] = M[p], M[c], inv[p], inv[c]
        f = M[c][c]
        M[c] = [v / f for v in M[c]]
        inv[c] = [v / f for v in inv[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                g = M[r][c]
                M[r] = [a - g * b for a, b in zip(M[r], M[c])]
                inv[r] = [a - g * b for a, b in zip(inv[r], inv[c])]
    Dn = 1
    for row in inv:
        for v in row:
            Dn = lcm(Dn, v.denominator)
    return [[int(v * Dn) for v in row] for row in inv], Dn


def solve_exact(xs, ys, poly: int):
    """The rational coefficients of the polynomial through the basis nodes (a list of Fraction), or None if fewer
    than poly points or two x-points are equal."""
    xs, ys = [int(x) for x in xs], [int(v) for v in ys]
    if len(xs) < poly or len(set(xs)) != len(xs):
        return None
    order = basis_order(xs, poly)
    A, Dn = inverse_vandermonde(tuple(xs[i] for i in order))
    return [Fraction(sum(A[j][i] * ys[order[i]] for i in range(poly)), Dn) for j in range(poly)]


def recover_ref(xs, ys, poly: int):
    """Exact recovery: the integer coefficients, or None if two x-points are equal, a coefficient is not an integer
    or leaves int64, or a share is off the polynomial."""
    c = solve_exact(xs, ys, poly)
    if c is None or any(v.denominator != 1 for v in c):
        return None
    c = [int(v) for v in c]
    if any(v < I64_MIN or v > I64_MAX for v in c):
        return None
    for x, yv in zip(xs, ys):
        acc = 0
        for v in reversed(c):
            acc = acc * int(x) + v
        if acc != int(yv):
            return None
    return c


POLY, NCH, T = 10, 17, 21
D_REC = NCH * POLY - 3
XS_ALL = list(range(-10, 11))
MASK = [1, 0, 1, 1, 0, 1]
LAYOUTS = {
    "all21": XS_ALL,
    "two_miners14": list(range(-10, -3)) + list(range(4, 11)),
    "one_to_ten": list(range(1, 11)),
    "npts_eq_poly": [-4, 4, -5, 5, -6, 6, -7, -8, -9, -10],
    "shuffled21": [int(v) for v in np.random.default_rng(21).permutation(XS_ALL)],
}
COEFF_SETS = ("uniform8e9", "c0_pm_max", "c0_min", "zero")


def _coeffs(cset: str) -> list:
    g = _rng("rc" + cset)
    if cset == "uniform8e9":
        c = [[int(v) for v in row] for row in g.integers(-8 * 10 ** 9, 8 * 10 ** 9, (NCH, POLY), endpoint=True)]
        # the two corners of the range: |y(10)| and |y(-10)| = 8e9 * 1111111111 = 0.9637 * 2^63
        c[0] = [8 * 10 ** 9] * POLY
        c[1] = [-8 * 10 ** 9 * (-1) ** j for j in range(POLY)]
        return c
    if cset == "uniform1e6":
        return [[int(v) for v in row] for row in g.integers(-10 ** 6, 10 ** 6, (NCH, POLY), endpoint=True)]
    c0 = {"c0_pm_max": lambda k: I64_MAX if k % 2 == 0 else -I64_MAX, "c0_min": lambda k: I64_MIN,
          "zero": lambda k: 0}[cset]
    return [[c0(k)] + [0] * (POLY - 1) for k in range(NCH)]


def _eval(c, x: int) -> int:
    acc = 0
    for v in reversed(c):
        acc = acc * x + v
    return acc


class RecCase(NamedTuple):
    name: str
    xs: list           # the layout's x-points, in column order
    cols: list         # their columns in the T = 21 share row (x + 10)
    coeffs: list       # [NCH][POLY] Python integers: the aggregate
    ys: np.ndarray     # int64 [R, NCH, T]: every row's shares at -10..10; rows with MASK = 0 are noise
    agg: np.ndarray    # int64 [NCH, npts]: the masked rows' sums at the layout's points
    W: np.ndarray      # fp64 [D_REC], non-zero


@lru_cache(maxsize=None)
def recovery_case(layout: str, cset: str) -> RecCase:
    """The aggregate's coefficients split over the four kept rows into parts of one sign (c = 4 q + r: q + r, q, q,
    q), so every partial row sum lies between 0 and the total; the two masked-out rows hold values near +-2^62."""
    g = _rng("rec" + layout + cset)
    xs = LAYOUTS[layout]
    coeffs = _coeffs(cset)
    R = len(MASK)
    ys = np.zeros((R, NCH, T), np.int64)
    kept = [r for r in range(R) if MASK[r]]
    for k in range(NCH):
        q = [int(Fraction(c, 4).__trunc__()) for c in coeffs[k]]
        parts = [[c - 3 * qq for c, qq in zip(coeffs[k], q)]] + [q] * 3
        for r, part in zip(kept, parts):
            for t, x in enumerate(XS_ALL):
                v = _eval(part, x)
                assert I64_MIN <= v <= I64_MAX
                ys[r, k, t] = v
    for r in range(R):
        if not MASK[r]:
            ys[r] = g.integers(-2 ** 62, 2 ** 62, (NCH, T))
    cols = [x + 10 for x in xs]
    agg = np.asarray([[_eval(coeffs[k], x) for x in xs] for k in range(NCH)], dtype=object)
    assert all(I64_MIN <= int(v) <= I64_MAX for v in agg.reshape(-1))
    W = g.standard_normal(D_REC)
    return RecCase(f"{layout}-{cset}", xs, cols, coeffs, ys, agg.astype(np.int64), W)


def w_expected(W: np.ndarray, coeffs, status=None) -> np.ndarray:
    """numpy's W + v / qscale, v the int64 coefficients as fp64 (0 where the chunk's status is 0)."""
    c = np.asarray(coeffs, dtype=object)
    if status is not None:
        c = c * np.asarray(status, dtype=object)[:, None]
    v = np.asarray([float(int(t)) for t in c.reshape(-1)][: W.size], np.float64)
    return W + v / QSCALE


TAMPER_CHUNKS = (3, 11)          # one in k_recover_w's block 0, one in block 1
TAMPER_ROW = 2                   # a kept row
X_NONBASIS, X_BASIS = 6, -2      # all21: the basis is 0, -1, 1, ..., -4, 4, -5


def tampers() -> list:
    """(name, x of the share, amount) on the all21 layout; Dn keeps the basis division exact."""
    _, Dn = inverse_vandermonde(tuple(LAYOUTS["all21"][i] for i in basis_order(LAYOUTS["all21"], POLY)))
    return [("nonbasis+1", X_NONBASIS, 1), ("nonbasis-1", X_NONBASIS, -1), ("basis+1", X_BASIS, 1),
            ("basis-1", X_BASIS, -1), ("basis+Dn", X_BASIS, Dn), ("basis-Dn", X_BASIS, -Dn)]


def tampered(case: RecCase, x: int, amount: int) -> np.ndarray:
    ys = case.ys.copy()
    for k in TAMPER_CHUNKS:
        v = int(ys[TAMPER_ROW, k, x + 10]) + amount
        assert I64_MIN <= v <= I64_MAX
        ys[TAMPER_ROW, k, x + 10] = v
    return ys


OVERFLOW_XS = list(range(1, 11))


@lru_cache(maxsize=None)
def overflow_case():
    """xs = 1..10, poly = 10, Dn = 9!: chunks 3 and 11 hold y_i = (-1)^(i-1) * floor(2^60 / Dn) * Dn -- shares of 61
    bits whose exact coefficients are integers of up to 72 bits; the other chunks are ordinary.
    Returns (agg int64 [NCH, 10], expected coefficients or None per chunk, W)."""
    g = _rng("overflow")
    _, Dn = inverse_vandermonde(tuple(OVERFLOW_XS))
    m = (2 ** 60 // Dn) * Dn
    coeffs = _coeffs("uniform1e6")
    agg = np.asarray([[_eval(c, x) for x in OVERFLOW_XS] for c in coeffs], np.int64)
    for k in TAMPER_CHUNKS:
        agg[k] = [(-1) ** (i - 1) * m for i in range(1, 11)]
    expect = [None if k in TAMPER_CHUNKS else coeffs[k] for k in range(NCH)]
    return agg, expect, g.standard_normal(D_REC)


def repeated_x_case():
    """Eleven points with x = 1 twice (equal shares there): every other point lies on one polynomial, and the basis
    holds both copies.  Returns (xs, agg int64 [NCH, 11], W)."""
    g = _rng("repeat")
    xs = [0, 1, 1, -1, 2, -2, 3, -3, 4, -4, 5]
    coeffs = _coeffs("uniform1e6")
    agg = np.asarray([[_eval(c, x) for x in xs] for c in coeffs], np.int64)
    return xs, agg, g.standard_normal(D_REC)
