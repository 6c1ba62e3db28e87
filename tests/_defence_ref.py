"""References and case lists of the single-verifier Krum (K5a-c) and LSH sieve (LS1-LS3) edge tests.

Nothing here runs torch or imports the code under test.  Integer inputs are handled in Python / numpy int64
integers (exact), real inputs with math.fsum over exactly representable terms (correctly rounded sums).

Why integers: the kernels read fp32 and accumulate in fp64 (Gram, distances, scores, weighted sum) or in fp32
(the LSH projections).  With small integer inputs every product and every partial sum is representable whatever
the summation order, so the kernels' results must EQUAL the integer ones: |Gram entry| < 2^53 and
sum_k |(x_k - mu_k) p_k| < 2^24 are the two conditions (exactness_margin below; tests/test_defence_ref_cpu.py
checks them for every generated input, on the CPU).

Every case list is built once per process and never modified; tests/test_defence_ref_cpu.py vets each case
against the project's CPU branches before tests/test_gpu_krum_lsh_edges.py takes it to the kernels.
"""
from __future__ import annotations

import math
import zlib
from functools import lru_cache
from typing import NamedTuple

import numpy as np

U64 = 2.0 ** -53          # unit roundoff of fp64


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def _ints(X) -> np.ndarray:
    """X as int64, refusing anything that is not integer-valued."""
    X = np.asarray(X)
    Xi = np.rint(X).astype(np.int64)
    assert np.array_equal(Xi.astype(np.float64), X.astype(np.float64)), "integer-valued input expected"
    return Xi


def is_integral(X) -> bool:
    X = np.asarray(X, np.float64)
    return bool(np.all(np.isfinite(X)) and np.array_equal(X, np.rint(X)))


# ---------------------------------------------------------------------------- Krum
def gram_int(X) -> np.ndarray:
    """Exact Gram of integer-valued rows: int64 [n, n] (the inputs of this file stay far below 2^63)."""
    Xi = _ints(X)
    assert Xi.size == 0 or int(np.abs(Xi).max()) ** 2 * max(1, Xi.shape[1]) < 2 ** 62
    return Xi @ Xi.T


def krum_select(dist, groupsize: int, n_accept: int):
    """The selection rule written on k_krum_scores / k_krum_accept, applied to given distances (rows of Python
    numbers): score_i = sum of the entries of row i whose rank lies in [1, groupsize-1), ties ranked by column
    index; the n_accept lowest scores are accepted, ties by row index.  Returns (scores list, accept int array)."""
    n = len(dist)
    scores = []
    for i in range(n):
        order = sorted(range(n), key=lambda j: (dist[i][j], j))
        kept = [dist[i][j] for j in order[1:max(1, groupsize - 1)]]
        scores.append(sum(kept) if all(isinstance(v, int) for v in kept) else math.fsum(kept))
    order = sorted(range(n), key=lambda i: (scores[i], i))
    accept = np.zeros(n, dtype=np.int32)
    accept[order[:max(0, n_accept)]] = 1
    return scores, accept


def krum_ref(X, groupsize: int, n_accept: int):
    """(dist [n, n], scores [n], accept int32 [n]) of Multi-Krum over the rows of X.

    Integer-valued X: int64 results, exact.  Real X (fp32 values): every distance is the correctly rounded
    sum_k x_ik^2 + x_jk^2 - 2 x_ik x_jk (each term is a product of two fp32 numbers, exact in fp64), every score
    the correctly rounded sum of its kept distances; float64 results."""
    X = np.asarray(X)
    n = X.shape[0]
    if is_integral(X):
        G = gram_int(X)
        dist = [[int(G[i, i] + G[j, j] - 2 * G[i, j]) for j in range(n)] for i in range(n)]
        scores, accept = krum_select(dist, groupsize, n_accept)
        return np.array(dist, dtype=np.int64).reshape(n, n), np.array(scores, dtype=np.int64), accept
    Xd = X.astype(np.float64)
    sq = Xd * Xd
    dist = [[0.0 if i == j else math.fsum(np.concatenate([sq[i], sq[j], -2.0 * Xd[i] * Xd[j]])) for j in range(n)]
            for i in range(n)]
    scores, accept = krum_select(dist, groupsize, n_accept)
    return np.array(dist, dtype=np.float64).reshape(n, n), np.array(scores, dtype=np.float64), accept


def krum_ref_rounded(X, groupsize: int, n_accept: int):
    """Multi-Krum where the fp64 roundings are part of the specification: integer rows with at most two nonzero
    coordinates per pair of rows, so every Gram entry is ONE correctly rounded sum of two exact products whatever
    the order (float(int) rounds to nearest even, as the hardware does), and D_ij = (G_ii + G_jj) - 2 G_ij in
    fp64 as K5b writes it.  Such distances can come out negative; the rule then still drops rank 0 only."""
    G = gram_int(X)
    n = G.shape[0]
    assert int((_ints(X) != 0).any(0).sum()) <= 2, "two nonzero columns at the most"
    Gf = [[float(int(G[i, j])) for j in range(n)] for i in range(n)]
    dist = [[(Gf[i][i] + Gf[j][j]) - 2.0 * Gf[i][j] for j in range(n)] for i in range(n)]
    scores, accept = krum_select(dist, groupsize, n_accept)
    return np.array(dist, dtype=np.float64).reshape(n, n), np.array(scores, dtype=np.float64), accept


def gram_bound(X, groupsize: int | None = None):
    """Error bounds of an fp64 Krum over real (fp32-valued) rows, against krum_ref: (gram, dist, score).

    gram [n, n]: gamma_D * sum_k |x_ik x_jk| with gamma_D = D u / (1 - D u), u = 2^-53: the products are exact and
    a sum of D terms in any order (split-K included) commits at most D roundings per path.
    dist [n, n]: D_ij = (G_ii + G_jj) - 2 G_ij inherits b_ii + b_jj + 2 b_ij and adds two roundings, each at most u
    times an intermediate no larger than S_ii + S_jj + 2 S_ij (S = sum_k |x_ik x_jk|) up to a factor 1 + gamma_D;
    the reference's own distance is correctly rounded (one more u |D_ij|).  4 u (S_ii + S_jj + 2 S_ij) covers the
    three.  The diagonal is exactly 0 on both sides.
    score [n] (groupsize given): the sum of the m = groupsize - 2 smallest off-diagonal entries of a row moves by
    at most the sum of the m largest distance bounds of that row when the entries move within their bounds
    (whichever entries end up kept), and summing at most n kept distances in fp64 adds (n + 2) u times their sum
    (the reference's fsum included)."""
    Xd = np.asarray(X).astype(np.float64)
    n, D = Xd.shape
    A = np.abs(Xd)
    S = np.array([[math.fsum(A[i] * A[j]) for j in range(n)] for i in range(n)], dtype=np.float64).reshape(n, n)
    gamma = D * U64 / (1.0 - D * U64)
    gb = gamma * S
    sd = np.diag(S)
    tot = sd[:, None] + sd[None, :] + 2.0 * S
    db = (np.diag(gb)[:, None] + np.diag(gb)[None, :] + 2.0 * gb) + 4.0 * U64 * tot
    np.fill_diagonal(db, 0.0)
    if groupsize is None:
        return gb, db, None
    m = max(0, min(groupsize - 2, n - 1))
    dist, _, _ = krum_ref(X, groupsize, 0)
    sb = np.zeros(n)
    for i in range(n):
        off = np.delete(np.arange(n), i)
        worst = np.sort(db[i, off])[::-1][:m]
        largest = np.sort(np.abs(dist[i, off]))[::-1][:m]
        sb[i] = math.fsum(worst) + (n + 2) * U64 * math.fsum(largest + worst)
    return gb, db, sb


def decided_rows(scores, bound) -> np.ndarray:
    """bool [n]: the rows whose reference score is further than twice the (largest) score bound from every other
    score -- their place in the ranking, and so their accept flag, cannot change within the bound."""
    s = np.asarray(scores, np.float64)
    gap = np.abs(s[:, None] - s[None, :])
    np.fill_diagonal(gap, np.inf)
    return gap.min(1) > 2.0 * float(np.max(bound)) if len(s) > 1 else np.ones(len(s), bool)


class KrumCase(NamedTuple):
    name: str
    X: np.ndarray          # fp32 [n, D], integer-valued
    groupsize: int
    n_accept: int
    ksplit: int


def _ix(name, n, D, lo=-8, hi=8) -> np.ndarray:
    return _rng(name).integers(lo, hi + 1, size=(n, D)).astype(np.float32)


KRUM_SHAPES = ((1, 1), (2, 3), (3, 4), (15, 31), (16, 32), (16, 4), (17, 33), (17, 257), (33, 3), (33, 32), (15, 33),
               (128, 1), (128, 31), (128, 257))
KRUM_KSPLITS = (4, 6, 32, 36, 256, 257, 357)          # at n = 17, D = 257: D and D + 100 are the last two
KRUM_GROUPSIZES = (2, 3, 17, 19, 27)                  # at n = 17: 2, 3, n, n + 2, n + 10
KRUM_NACCEPTS = (0, 1, 16, 17, 22)                    # at n = 17: 0, 1, n - 1, n, n + 5


@lru_cache(maxsize=None)
def krum_shape_cases() -> tuple:
    out = []
    for n, D in KRUM_SHAPES:
        name = f"n{n}_D{D}"
        out.append(KrumCase(name, _ix(name, n, D), max(2, n - n // 4), (n + 1) // 2, 256 if D != 33 else 8))
    return tuple(out)


@lru_cache(maxsize=None)
def krum_ksplit_cases() -> tuple:
    X = _ix("ksplit", 17, 257)
    return tuple(KrumCase(f"ksplit{k}", X, 12, 8, k) for k in KRUM_KSPLITS)


@lru_cache(maxsize=None)
def krum_window_cases() -> tuple:
    X = _ix("window", 17, 33)
    return tuple(KrumCase(f"g{g}_a{a}", X, g, a, 8) for g in KRUM_GROUPSIZES for a in KRUM_NACCEPTS)


@lru_cache(maxsize=None)
def krum_tie_cases() -> tuple:
    same = np.tile(_ix("same", 1, 33), (17, 1))
    dup = _ix("dup", 17, 33)
    dup[11] = dup[3]
    dup[16] = dup[3]
    dup[5] = dup[4]
    sym = np.zeros((17, 8), np.float32)                 # +-3 e_k and the origin: 16 equal scores and one lower
    for k in range(8):
        sym[2 * k, k], sym[2 * k + 1, k] = 3.0, -3.0
    line = np.zeros((33, 1), np.float32)                # equally spaced collinear points: mirrored scores are equal
    line[:, 0] = np.arange(33) - 16
    return (KrumCase("identical", same, 9, 6, 8), KrumCase("identical_all", same, 30, 17, 256),
            KrumCase("duplicates", dup, 10, 9, 16), KrumCase("duplicates_g3", dup, 3, 4, 256),
            KrumCase("symmetric", sym, 6, 5, 4), KrumCase("symmetric_g17", sym, 17, 16, 3),
            KrumCase("collinear", line, 7, 12, 256))


def krum_int_cases() -> tuple:
    return krum_shape_cases() + krum_ksplit_cases() + krum_window_cases() + krum_tie_cases()


@lru_cache(maxsize=None)
def krum_refs() -> dict:
    return {c.name: krum_ref(c.X, c.groupsize, c.n_accept) for c in krum_int_cases()}


@lru_cache(maxsize=None)
def krum_rounded_case() -> KrumCase:
    """Rows (2^28, q): G = 2^56 + q q' rounds to a multiple of 16 (ties to even), and D_ij of the pairs (6, 7) and
    (-7, -6) comes out as -32 where the true squared distance is 1."""
    X = np.zeros((9, 5), np.float32)
    X[:, 1] = 2.0 ** 28
    X[:, 3] = (0, 6, 7, -7, -6, 3, 12, 1, -12)
    return KrumCase("rounded_negative", X, 5, 4, 256)


KRUM_REAL = dict(n=40, D=300, groupsize=22, n_accept=20, ksplit=64, seed=20240)


@lru_cache(maxsize=None)
def krum_real_case() -> KrumCase:
    k = KRUM_REAL
    X = np.random.default_rng(k["seed"]).standard_normal((k["n"], k["D"])).astype(np.float32)
    return KrumCase("real", X, k["groupsize"], k["n_accept"], k["ksplit"])


@lru_cache(maxsize=None)
def krum_real_ref():
    """(dist, scores, accept, dist bound, score bound, decided rows) of the real-valued case."""
    c = krum_real_case()
    dist, scores, accept = krum_ref(c.X, c.groupsize, c.n_accept)
    _, db, sb = gram_bound(c.X, c.groupsize)
    return dist, scores, accept, db, sb, decided_rows(scores, sb)


# ---------------------------------------------------------------------------- LSH codes (LS1)
def lsh_codes_ref(X, mu, planes, L: int, K: int) -> np.ndarray:
    """uint32 [n, L]: bit b of table t is set iff <x - mu, planes[t * K + b]> > 0, strictly.  Integer inputs."""
    V = _ints(X) - _ints(mu)[None, :]
    P = _ints(planes)
    assert P.shape[0] >= L * K and 0 < K <= 32
    proj = V @ P[:L * K].T                                       # int64, exact
    out = np.zeros((V.shape[0], L), dtype=np.uint32)
    for t in range(L):
        for b in range(K):
            out[:, t] |= (proj[:, t * K + b] > 0).astype(np.uint32) << np.uint32(b)
    return out


class CodesCase(NamedTuple):
    name: str
    X: np.ndarray          # fp32 [n, D] integers in [-8, 8]
    mu: np.ndarray         # fp32 [D] integers in [-8, 8]
    planes: np.ndarray     # fp32 [L * K, D] integers in [-4, 4]
    L: int
    K: int


LSH_LK = ((1, 1), (4, 12), (2, 32), (64, 1), (4, 16), (3, 7))
LSH_D = (1, 5, 255, 256, 257, 600)
LSH_N = (1, 3, 70)


@lru_cache(maxsize=None)
def lsh_codes_cases() -> tuple:
    out = []
    for a, (L, K) in enumerate(LSH_LK):
        for b, D in enumerate(LSH_D):
            n = LSH_N[(a + b) % 3]
            name = f"L{L}_K{K}_D{D}_n{n}"
            r = _rng(name)
            X = r.integers(-8, 9, size=(n, D)).astype(np.float32)
            mu = r.integers(-8, 9, size=(D,)).astype(np.float32)
            X[0] = mu                                            # a row equal to mu: every bit 0
            P = r.integers(-4, 5, size=(L * K, D)).astype(np.float32)
            out.append(CodesCase(name, X, mu, P, L, K))
    return tuple(out)


@lru_cache(maxsize=None)
def lsh_codes_planted() -> tuple:
    """Hand-made rows.  Each entry: (case, expected uint32 codes [n, L])."""
    out = []
    # D = 5, one table of 3 bits: row 1 is orthogonal to plane 1 through cancellation, positive on planes 0 and 2
    mu = np.array([1, -2, 0, 3, 0], np.float32)
    P = np.array([[1, 0, 0, 0, 0], [1, -1, 0, 0, 0], [0, 0, 1, 0, 0]], np.float32)
    V = np.array([[0, 0, 0, 0, 0], [2, 2, 1, 0, 0], [-1, 0, -1, 0, 0]], np.float32)
    out.append((CodesCase("orth_D5", V + mu, mu, P, 1, 3), np.array([[0], [0b101], [0]], np.uint32)))
    # D = 600: plane 1 alternates +-1, so <1, p1> is 0 only once the 256 threads' partial sums have met
    D = 600
    mu = np.full(D, 2, np.float32)
    P = np.ones((3, D), np.float32)
    P[1, 1::2] = -1
    V = np.stack([np.zeros(D), np.ones(D), -np.ones(D)]).astype(np.float32)
    V2 = V.copy()
    V2[1, 0] = 2                                                 # one more on a +1 column: plane 1 turns positive
    out.append((CodesCase("orth_D600", V + mu, mu, P, 1, 3), np.array([[0], [0b101], [0]], np.uint32)))
    out.append((CodesCase("orth_D600_plus1", V2 + mu, mu, P, 1, 3), np.array([[0], [0b111], [0]], np.uint32)))
    # K = 32: plane 31 of table 0 and plane 63 (bit 31 of table 1)
    D = 257
    mu = np.zeros(D, np.float32)
    P = np.zeros((64, D), np.float32)
    for q in range(64):
        P[q, q] = 1
    P[31, 256], P[63, 256] = 4, -4
    X = np.zeros((3, D), np.float32)
    X[0, 256] = 1                                                # bit 31 of table 0 only
    X[1, 256] = -1                                               # bit 31 of table 1 only
    X[2, :64] = 1                                                # every bit
    X[2, 63] = 0                                                 # ... except bit 31 of table 1 (exactly 0)
    out.append((CodesCase("bit31", X, mu, P, 2, 32),
                np.array([[0x80000000, 0], [0, 0x80000000], [0xFFFFFFFF, 0x7FFFFFFF]], np.uint32)))
    return tuple(out)


# ---------------------------------------------------------------------------- LSH count (LS2)
def lsh_count_ref(G, codes, L: int, rows, thr: float) -> np.ndarray:
    """int32 [m]: for each listed row i, the number of listed rows j that are a candidate (L == 0: every row;
    else equal to i's code in at least one table, or i itself) and satisfy j == i or d2 < thr, with
    d2 = G_ii + G_jj - 2 G_ij.  An integer G is compared as Python integers against the float thr (exact)."""
    G = np.asarray(G)
    exact = np.issubdtype(G.dtype, np.integer)
    rows = [int(r) for r in rows]
    cd = None if L == 0 else np.asarray(codes).view(np.uint32).reshape(-1, L)
    out = np.zeros(len(rows), dtype=np.int32)
    for a, i in enumerate(rows):
        c = 0
        for j in rows:
            if j == i:
                c += 1
                continue
            if L and not any(cd[i, t] == cd[j, t] for t in range(L)):
                continue
            d2 = (int(G[i, i]) + int(G[j, j]) - 2 * int(G[i, j])) if exact else \
                (float(G[i, i]) + float(G[j, j]) - 2.0 * float(G[i, j]))
            c += d2 < thr
        out[a] = c
    return out


class CountCase(NamedTuple):
    name: str
    X: np.ndarray          # fp32 [U, D], integer-valued
    codes: np.ndarray      # uint32 [U, L]
    L: int
    rows: tuple
    thr: float


def _count_X(name, U, D=6) -> np.ndarray:
    return _rng(name).integers(-3, 4, size=(U, D)).astype(np.float32)


def _d2(X, i, j) -> int:
    v = _ints(X[i]) - _ints(X[j])
    return int(v @ v)


@lru_cache(maxsize=None)
def lsh_count_cases() -> tuple:
    out = []
    nocodes = lambda U: np.zeros((U, 0), np.uint32)                     # noqa: E731
    for U in (1, 16, 17, 300):
        X = _count_X(f"U{U}", U)
        r = _rng(f"codes{U}")
        cd1 = r.choice(np.array([0, 1, 2, 0x80000000], np.uint32), size=(U, 1))
        out.append(CountCase(f"U{U}_all_L0", X, nocodes(U), 0, tuple(range(U)), 9.0))
        out.append(CountCase(f"U{U}_all_L1", X, cd1, 1, tuple(range(U)), 30.0))
    X = _count_X("U300", 300)
    r = _rng("subsets")
    cd4 = r.integers(0, 3, size=(300, 4)).astype(np.uint32)
    cd4[:, 3] |= np.uint32(0x80000000)
    perm = tuple(int(v) for v in r.permutation(300))
    out.append(CountCase("U300_257rows_L0", X, nocodes(300), 0, perm[:257], 12.0))
    out.append(CountCase("U300_257rows_L4", X, cd4, 4, perm[:257], 40.0))
    out.append(CountCase("U300_shuffled100_L0", X, nocodes(300), 0, perm[100:200], 12.0))
    out.append(CountCase("U300_shuffled100_L4", X, cd4, 4, perm[200:300], 40.0))
    hilo = tuple(range(290, 300)) + tuple(range(0, 10)) + (40, 41, 160, 17)
    out.append(CountCase("U300_high_tile_first_L0", X, nocodes(300), 0, hilo, 20.0))
    out.append(CountCase("U300_high_tile_first_L4", X, cd4, 4, hilo, 60.0))
    # thr on an integer d2: strict <, and one ulp above
    d = float(_d2(X, 290, 3))
    assert d > 0
    out.append(CountCase("thr_equal_L0", X, nocodes(300), 0, hilo, d))
    out.append(CountCase("thr_ulp_above_L0", X, nocodes(300), 0, hilo, float(np.nextafter(d, np.inf))))
    out.append(CountCase("thr_ulp_below_L0", X, nocodes(300), 0, hilo, float(np.nextafter(d, -np.inf))))
    return tuple(out)


@lru_cache(maxsize=None)
def lsh_count_planted() -> tuple:
    """L = 4, every row alone in every bucket but for planted pairs.  (case, expected counts)."""
    U = 40
    X = np.zeros((U, 6), np.float32)
    X[:, 0] = 10 * np.arange(U)                                       # far apart: d2 >= 100
    X[21], X[5] = X[20], X[4]                                          # exact duplicates (d2 = 0)
    X[31] = X[30]
    X[31, 1] = 3                                                       # d2 = 9
    cd = (np.arange(U, dtype=np.uint32)[:, None] + np.uint32(1000) * np.arange(1, 5, dtype=np.uint32)[None, :])
    cd[21, 3] = cd[20, 3]           # collide in the last table only, within thr: counted
    cd[31, 3] = cd[30, 3]           # d2 = 9: counted only while thr > 9
    cd[11, 0] = cd[10, 0]           # share a bucket, d2 = 100: beyond thr, not counted
    #                                 rows 4, 5: duplicates that share no bucket: not counted
    rows = tuple(range(U - 1, -1, -1))

    def expect(pairs):
        e = np.ones(U, np.int32)
        for p in pairs:
            e[[rows.index(v) for v in p]] = 2
        return e
    return ((CountCase("planted_thr50", X, cd, 4, rows, 50.0), expect([(20, 21), (30, 31)])),
            (CountCase("planted_thr9", X, cd, 4, rows, 9.0), expect([(20, 21)])),
            (CountCase("planted_thr9ulp", X, cd, 4, rows, float(np.nextafter(9.0, np.inf))), expect([(20, 21), (30, 31)])),
            (CountCase("planted_thr101", X, cd, 4, rows, 101.0), expect([(20, 21), (30, 31), (10, 11)])))


class SieveCase(NamedTuple):
    name: str
    X: np.ndarray          # fp32 [U, D], integer-valued, with planted duplicates
    inboxes: tuple         # overlapping row lists of different lengths
    thr: float


@lru_cache(maxsize=None)
def sieve_cases() -> tuple:
    U, D = 50, 20
    X = _rng("sieve").integers(-2, 3, size=(U, D)).astype(np.float32)
    X[7], X[33], X[41] = X[2], X[2], X[40]
    a = (2, 7, 33, 40, 41) + tuple(range(10, 30))
    b = (49, 33, 7, 3, 2) + tuple(range(20, 48, 3))
    return (SieveCase("dups_thr70", X, (a, b), 70.0), SieveCase("dups_thr1_over_d", X, (a, b), 1.0 / D))


# ---------------------------------------------------------------------------- weighted rows (LS3)
def _split(w: float):
    """w = hi + lo with at most 26 significant bits each (Veltkamp), so hi * x and lo * x are exact for fp32 x."""
    c = 134217729.0 * w
    hi = c - (c - w)
    return hi, w - hi


def weighted_rows_ref(X, w) -> np.ndarray:
    """float64 [D]: sum_i w_i x_ik, fsum per column over exactly representable terms (correctly rounded)."""
    Xd = np.asarray(X).astype(np.float64)
    n, D = Xd.shape
    parts = [_split(float(v)) for v in np.asarray(w, np.float64)]
    hi, lo = np.array([p[0] for p in parts]), np.array([p[1] for p in parts])
    assert np.array_equal(hi + lo, np.asarray(w, np.float64))
    H, Lo = hi[:, None] * Xd, lo[:, None] * Xd
    return np.array([math.fsum(np.concatenate([H[:, k], Lo[:, k]])) for k in range(D)], dtype=np.float64)


def weighted_rows_bound(X, w) -> np.ndarray:
    """float64 [D]: n u sum_i |w_i x_ik| -- n products and adds of one rounding each, to first order."""
    Xd = np.abs(np.asarray(X).astype(np.float64))
    wa = np.abs(np.asarray(w, np.float64))
    return Xd.shape[0] * U64 * np.array([math.fsum(wa * Xd[:, k]) for k in range(Xd.shape[1])])


class WeightedCase(NamedTuple):
    name: str
    X: np.ndarray          # fp32 [n, D]
    cnt: np.ndarray        # int32 [n]: w = 1 / cnt


WEIGHTED_D = (1, 255, 256, 257)
WEIGHTED_N = (1, 2, 70)


@lru_cache(maxsize=None)
def weighted_int_cases() -> tuple:
    out = []
    for n in WEIGHTED_N:
        for D in WEIGHTED_D:
            name = f"w_n{n}_D{D}"
            r = _rng(name)
            out.append(WeightedCase(name, r.integers(-8, 9, size=(n, D)).astype(np.float32),
                                    r.choice(np.array([1, 2, 4, 8], np.int32), size=n)))
    return tuple(out)


@lru_cache(maxsize=None)
def weighted_real_case() -> WeightedCase:
    r = _rng("w_real")
    return WeightedCase("w_real", r.standard_normal((70, 257)).astype(np.float32),
                        r.choice(np.array([3, 5, 7], np.int32), size=70))


# ---------------------------------------------------------------------------- exactness
def exactness_margin() -> dict:
    """The largest |Gram entry| (must stay < 2^53) and the largest sum_k |(x_k - mu_k) p_k| (must stay < 2^24:
    it bounds every fp32 partial sum of a projection) over every integer input the GPU tests use."""
    gram, proj, wsum = 0, 0, 0.0
    for c in krum_int_cases():
        Xi = np.abs(_ints(c.X))
        gram = max(gram, int((Xi @ Xi.T).max()))
    for c in lsh_count_cases() + tuple(p[0] for p in lsh_count_planted()) + sieve_cases():
        Xi = np.abs(_ints(c.X))
        gram = max(gram, int((Xi @ Xi.T).max()))
    for c in lsh_codes_cases() + tuple(p[0] for p in lsh_codes_planted()):
        V = np.abs(_ints(c.X) - _ints(c.mu)[None, :])
        proj = max(proj, int((V @ np.abs(_ints(c.planes)).T).max()))
    for c in weighted_int_cases():
        # multiples of 1/8 below 2^53 / 8 add exactly
        wsum = max(wsum, float((np.abs(c.X.astype(np.float64)) / c.cnt[:, None]).sum(0).max()))
    return {"gram": gram, "proj": proj, "weighted": wsum}
