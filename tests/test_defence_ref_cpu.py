"""The references of tests/_defence_ref.py, without a GPU: hand-checked cases, agreement with the project's CPU
branches (ops.ml.krum, lsh.codes, lsh.neighbour_counts, lsh.lsh_sieve) on integer inputs, and the exactness
preconditions of every input that tests/test_gpu_krum_lsh_edges.py takes to the kernels."""
import math

import numpy as np
import pytest
import torch

import _defence_ref as R
from biscotti_amd.ops import lsh
from biscotti_amd.ops import ml as K


# ---------------------------------------------------------------------------- hand-checked
def test_krum_three_collinear_points():
    X = np.array([[0.0], [1.0], [3.0]], np.float32)
    dist, scores, accept = R.krum_ref(X, 3, 1)              # groupsize 3: the single nearest neighbour
    assert dist.tolist() == [[0, 1, 9], [1, 0, 4], [9, 4, 0]]
    assert scores.tolist() == [1, 1, 4]
    assert accept.tolist() == [1, 0, 0]                     # 0 and 1 tie: the lower index wins
    assert R.krum_ref(X, 3, 2)[2].tolist() == [1, 1, 0]
    assert R.krum_ref(X, 4, 1)[1].tolist() == [10, 5, 13]   # both neighbours
    assert R.krum_ref(X, 4, 1)[2].tolist() == [0, 1, 0]
    assert R.krum_ref(X, 9, 1)[1].tolist() == [10, 5, 13]   # a window past n keeps what there is
    assert R.gram_int(X).tolist() == [[0, 0, 0], [0, 1, 3], [0, 3, 9]]


def test_krum_identical_rows_groupsize_and_n_accept_edges():
    X = np.tile(np.array([[2.0, -1.0, 5.0]], np.float32), (5, 1))
    dist, scores, accept = R.krum_ref(X, 4, 2)
    assert not dist.any() and scores.tolist() == [0] * 5
    assert accept.tolist() == [1, 1, 0, 0, 0]               # all tied: the first n_accept indices
    Y = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0], [0.0, -1.0]], np.float32)
    assert R.krum_ref(Y, 2, 4)[1].tolist() == [0, 0, 0, 0]  # groupsize 2: an empty window
    assert R.krum_ref(Y, 3, 4)[1].tolist() == [1, 25, 25, 1]
    assert R.krum_ref(Y, 3, 0)[2].tolist() == [0, 0, 0, 0]
    assert R.krum_ref(Y, 3, 9)[2].tolist() == [1, 1, 1, 1]
    assert R.krum_ref(Y, 3, 3)[2].tolist() == [1, 1, 0, 1]  # 25 == 25: row 1 before row 2
    assert R.krum_ref(Y, 1, 1)[1].tolist() == [0, 0, 0, 0] and R.krum_ref(Y, 0, 1)[1].tolist() == [0, 0, 0, 0]
    one = R.krum_ref(np.array([[7.0, 7.0]], np.float32), 5, 1)
    assert one[0].tolist() == [[0]] and one[1].tolist() == [0] and one[2].tolist() == [1]


def test_krum_real_path_is_the_integer_path_on_integers_and_rounds_correctly():
    X = R.krum_shape_cases()[6].X                            # 17 x 33
    d_i, s_i, a_i = R.krum_ref(X, 9, 5)
    d_r, s_r, a_r = R.krum_ref((X / 8).astype(np.float32), 9, 5)   # exact scaling: the same problem, real entries
    assert d_r.dtype == np.float64 and np.array_equal(d_r * 64, d_i) and np.array_equal(s_r * 64, s_i)
    assert np.array_equal(a_r, a_i)
    from fractions import Fraction
    Y = np.random.default_rng(1).standard_normal((4, 50)).astype(np.float32)
    d, _, _ = R.krum_ref(Y, 3, 1)
    for i in range(4):
        for j in range(4):
            ex = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(Y[i], Y[j]))
            assert d[i, j] == float(ex)                      # Fraction -> float rounds to nearest even


def test_krum_rounded_case_has_negative_distances():
    c = R.krum_rounded_case()
    dist, scores, accept = R.krum_ref_rounded(c.X, c.groupsize, c.n_accept)
    assert dist[1, 2] == -32.0 and dist[3, 4] == -32.0 and (np.diag(dist) == 0).all()
    assert np.array_equal(dist, dist.T)
    # row 1 (q = 6): sorted -32 (q = 7), 0 (itself), then the rest: ranks 1..3 keep the 0, not the -32
    row = sorted(dist[1].tolist())
    assert row[0] == -32.0 and row[1] == 0.0 and scores[1] == row[1] + row[2] + row[3]
    acc_cpu, sc_cpu = K.krum(torch.from_numpy(c.X), c.groupsize, c.n_accept)
    assert np.array_equal(sc_cpu.numpy(), scores) and np.array_equal(acc_cpu.numpy().astype(np.int32), accept)


def test_lsh_codes_planted_rows():
    for c, want in R.lsh_codes_planted():
        got = R.lsh_codes_ref(c.X, c.mu, c.planes, c.L, c.K)
        assert got.dtype == np.uint32 and np.array_equal(got, want), c.name
    # a projection of exactly 0 leaves its bit clear (strict >), its neighbours stay set
    c, want = R.lsh_codes_planted()[0]
    proj = (c.X - c.mu).astype(np.int64) @ c.planes.astype(np.int64).T
    assert proj[1].tolist() == [2, 0, 1] and want[1, 0] == 0b101


def test_lsh_count_hand_cases():
    X = np.array([[0, 0], [3, 0], [0, 4], [3, 0]], np.float32)      # d2: 01 = 9, 02 = 16, 12 = 25, 13 = 0
    G = R.gram_int(X)
    assert R.lsh_count_ref(G, None, 0, [0, 1, 2, 3], 9.0).tolist() == [1, 2, 1, 2]     # d2 == thr: not counted
    assert R.lsh_count_ref(G, None, 0, [0, 1, 2, 3], float(np.nextafter(9.0, 10.0))).tolist() == [3, 3, 1, 3]
    assert R.lsh_count_ref(G, None, 0, [0, 1, 2, 3], 16.5).tolist() == [4, 3, 2, 3]
    assert R.lsh_count_ref(G, None, 0, [2, 0], 16.5).tolist() == [2, 2]                # a listed subset, permuted
    assert R.lsh_count_ref(G, None, 0, [3], 100.0).tolist() == [1]
    cd = np.array([[1, 5, 9], [2, 6, 9], [3, 7, 11], [4, 8, 12]], np.uint32)          # 0 and 1 meet in table 2 only
    assert R.lsh_count_ref(G, cd, 3, [0, 1, 2, 3], 100.0).tolist() == [2, 2, 1, 1]
    assert R.lsh_count_ref(G, cd, 3, [0, 1, 2, 3], 9.0).tolist() == [1, 1, 1, 1]       # in a bucket, beyond thr
    assert R.lsh_count_ref(G, cd[:, :2], 2, [0, 1, 2, 3], 100.0).tolist() == [1, 1, 1, 1]   # near, no bucket
    for c, want in R.lsh_count_planted():
        assert R.lsh_count_ref(R.gram_int(c.X), c.codes, c.L, c.rows, c.thr).tolist() == want.tolist(), c.name


def test_weighted_rows_ref_is_correctly_rounded():
    from fractions import Fraction
    c = R.weighted_real_case()
    X, w = c.X[:9, :5], 1.0 / c.cnt[:9].astype(np.float64)
    got = R.weighted_rows_ref(X, w)
    for k in range(5):
        assert got[k] == float(sum(Fraction(float(w[i])) * Fraction(float(X[i, k])) for i in range(9)))
    assert R.weighted_rows_ref(np.array([[1, 2], [3, 5]], np.float32), [0.5, 0.25]).tolist() == [1.25, 2.25]


def test_gram_bound_dominates_a_plain_fp64_gram():
    c = R.krum_real_case()
    gb, db, sb = R.gram_bound(c.X, c.groupsize)
    Xd = c.X.astype(np.float64)
    G = Xd @ Xd.T
    ex = np.array([[math.fsum(Xd[i] * Xd[j]) for j in range(len(Xd))] for i in range(len(Xd))])
    assert (np.abs(G - ex) <= gb).all() and (gb > 0).all() and (gb < 1e-10).all()
    assert (np.diag(db) == 0).all() and (db >= 0).all() and (sb > 0).all() and sb.max() < 1e-8


# ---------------------------------------------------------------------------- the CPU branches
@pytest.mark.parametrize("case", R.krum_int_cases(), ids=lambda c: c.name)
def test_krum_ref_matches_cpu_branch(case):
    dist, scores, accept = R.krum_refs()[case.name]
    acc, sc = K.krum(torch.from_numpy(case.X), case.groupsize, case.n_accept)
    assert np.array_equal(sc.numpy(), scores.astype(np.float64))
    assert np.array_equal(acc.numpy().astype(np.int32), accept)
    assert np.array_equal(dist, dist.T) and not np.diag(dist).any() and (dist >= 0).all()
    assert accept.sum() == min(max(case.n_accept, 0), len(accept))


def test_krum_tie_cases_are_ties():
    refs = R.krum_refs()
    _, s, a = refs["identical"]
    assert not s.any() and a.tolist() == [1] * 6 + [0] * 11
    assert refs["identical_all"][2].tolist() == [1] * 17
    _, s, a = refs["symmetric"]
    assert len(set(s[:16].tolist())) == 1 and s[16] < s[0] and a.tolist() == [1, 1, 1, 1] + [0] * 12 + [1]
    d, s, _ = refs["duplicates"]
    assert d[3, 11] == 0 and d[3, 16] == 0 and d[4, 5] == 0 and s[3] == s[11] == s[16]
    _, s, _ = refs["collinear"]
    assert s.tolist() == s[::-1].tolist()
    # random small-D shapes are full of equal distances and equal scores too
    _, s, _ = refs["n128_D1"]
    assert len(set(s.tolist())) < 128


@pytest.mark.parametrize("case", R.lsh_codes_cases() + tuple(p[0] for p in R.lsh_codes_planted()),
                         ids=lambda c: c.name)
def test_lsh_codes_ref_matches_cpu_branch(case):
    c = case
    want = R.lsh_codes_ref(c.X, c.mu, c.planes, c.L, c.K)
    got = lsh.codes(torch.from_numpy(c.X), torch.from_numpy(c.mu), torch.from_numpy(c.planes), c.L, c.K)
    assert got.dtype == torch.int32
    assert np.array_equal(got.numpy().view(np.uint32), want)
    if np.array_equal(c.X[0], c.mu):
        assert not want[0].any()                              # a row equal to mu: every bit 0


def test_lsh_codes_cases_cover_the_edges():
    cases = R.lsh_codes_cases()
    assert {(c.L, c.K) for c in cases} == set(R.LSH_LK) and {c.X.shape[1] for c in cases} == set(R.LSH_D)
    assert {c.X.shape[0] for c in cases} == set(R.LSH_N)
    zero = bit31 = 0
    for c in cases:
        proj = (c.X - c.mu).astype(np.int64) @ c.planes.astype(np.int64).T
        zero += int((proj[1:] == 0).sum())
        if c.K == 32:
            bit31 += int((R.lsh_codes_ref(c.X, c.mu, c.planes, c.L, c.K) >> np.uint32(31)).sum())
    assert zero > 50 and bit31 > 20                            # exact zeros off row 0, and bit 31 in use


@pytest.mark.parametrize("case", R.sieve_cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("tables", [0, 4])
def test_lsh_count_ref_matches_cpu_branch(case, tables):
    X = torch.from_numpy(case.X)
    G = R.gram_int(case.X)
    got = lsh.neighbour_counts(X, case.thr, [list(r) for r in case.inboxes], tables=tables, bits=6, seed=11)
    cd = None
    if tables:
        cd = lsh.codes(X, X.mean(0), lsh.planes(tables, 6, X.shape[1], 11, "cpu"), tables, 6).numpy()
    for rows, g in zip(case.inboxes, got):
        want = R.lsh_count_ref(G, cd, tables, rows, case.thr)
        assert g.tolist() == want.tolist()
        assert want.max() > 1                                  # the planted duplicates are seen
    acc = lsh.sieve_accept(X, [list(r) for r in case.inboxes[:1]], X.shape[1], tables=tables, bits=6, seed=11)
    want = R.lsh_count_ref(G, cd, tables, case.inboxes[0], 1.0 / X.shape[1]) == 1
    assert acc[0].tolist() == want.tolist() and not want.all() and want.any()


@pytest.mark.parametrize("case", R.lsh_count_cases(), ids=lambda c: c.name)
def test_lsh_count_cases_against_cpu_arithmetic(case):
    """The same counts from the project's own CPU formula (fp64 Gram of integers: exact)."""
    c = case
    G = K._gram_exact_order(torch.from_numpy(c.X))
    r = torch.tensor(c.rows, dtype=torch.long)
    sq = torch.diagonal(G)
    d2 = sq[r][:, None] + sq[r][None, :] - 2.0 * G[r][:, r]
    cd = torch.from_numpy(c.codes.astype(np.int64))
    cand = torch.ones((len(r), len(r)), dtype=torch.bool) if c.L == 0 else \
        (cd[r][:, None, :] == cd[r][None, :, :]).any(-1)
    near = cand & (d2 < c.thr)
    near.fill_diagonal_(True)
    want = R.lsh_count_ref(R.gram_int(c.X), c.codes, c.L, c.rows, c.thr)
    assert near.sum(1).tolist() == want.tolist()


def test_lsh_count_cases_cover_the_edges():
    cases = {c.name: c for c in R.lsh_count_cases()}
    assert {len(c.rows) for c in cases.values()} >= {1, 16, 17, 257, 300}
    hi = cases["U300_high_tile_first_L0"].rows
    assert hi[0] >> 4 > hi[10] >> 4                             # gram_at meets ta > tb
    eq, up, dn = (R.lsh_count_ref(R.gram_int(cases[k].X), None, 0, cases[k].rows, cases[k].thr)
                  for k in ("thr_equal_L0", "thr_ulp_above_L0", "thr_ulp_below_L0"))
    assert (up >= eq).all() and (up > eq).any() and eq.tolist() == dn.tolist()
    assert up[hi.index(290)] > eq[hi.index(290)]


@pytest.mark.parametrize("case", R.weighted_int_cases(), ids=lambda c: c.name)
def test_weighted_rows_ref_on_integers(case):
    w = 1.0 / case.cnt.astype(np.float64)
    want = R.weighted_rows_ref(case.X, w)
    assert np.array_equal(want, (w[:, None] * case.X.astype(np.float64)).sum(0))       # exact: any order
    assert np.array_equal(want * 8, np.rint(want * 8))


def test_sieve_cpu_branch_on_the_sybil_sample():
    from test_lsh import _sample
    X = torch.from_numpy(_sample()).float()
    grad, cnt = lsh.lsh_sieve(X, tables=0)
    assert (cnt[-10:] == 10).all()
    w = 1.0 / cnt.double().numpy()
    assert (np.abs(grad.numpy() - R.weighted_rows_ref(X.numpy(), w)) <= R.weighted_rows_bound(X.numpy(), w)).all()


# ---------------------------------------------------------------------------- preconditions of the GPU tests
def test_every_gpu_input_is_exact():
    m = R.exactness_margin()
    print(m)
    assert 0 < m["gram"] < 2 ** 53 and 0 < m["proj"] < 2 ** 24 and 0 < m["weighted"] < 2 ** 50
    for c in R.krum_int_cases():
        assert R.is_integral(c.X) and c.X.dtype == np.float32 and np.abs(c.X).max() <= 16 and c.X.shape[1] <= 4096
    for c in R.lsh_codes_cases():
        assert np.abs(c.X).max() <= 8 and np.abs(c.mu).max() <= 8 and np.abs(c.planes).max() <= 4
        assert R.is_integral(c.X) and R.is_integral(c.mu) and R.is_integral(c.planes)
        assert c.L * c.K <= 64 and c.planes.shape == (c.L * c.K, c.X.shape[1])
    for c in R.lsh_count_cases() + tuple(p[0] for p in R.lsh_count_planted()):
        assert R.is_integral(c.X) and c.codes.shape == (len(c.X), c.L) and c.codes.dtype == np.uint32
        assert all(0 <= r < len(c.X) for r in c.rows) and len(set(c.rows)) == len(c.rows)


def test_krum_cases_cover_the_issue_grid():
    shapes = {c.X.shape for c in R.krum_shape_cases()}
    assert {s[0] for s in shapes} == {1, 2, 3, 15, 16, 17, 33, 128}
    assert {s[1] for s in shapes} == {1, 3, 4, 31, 32, 33, 257}
    assert any(n == 17 and D % 4 for n, D in shapes) and any(n == 128 and D % 4 for n, D in shapes)
    assert [c.ksplit for c in R.krum_ksplit_cases()] == [4, 6, 32, 36, 256, 257, 357]
    assert all(c.X.shape == (17, 257) for c in R.krum_ksplit_cases())
    assert len(R.krum_window_cases()) == 25 and all(len(c.X) == 17 for c in R.krum_window_cases())
    names = [c.name for c in R.krum_int_cases()]
    assert len(set(names)) == len(names)


def test_krum_real_case_leaves_no_row_undecided():
    c = R.krum_real_case()
    assert c.X.shape == (40, 300) and not R.is_integral(c.X)
    dist, scores, accept, db, sb, decided = R.krum_real_ref()
    gaps = np.sort(np.diff(np.sort(scores)))
    print("score bound max", sb.max(), "smallest score gap", gaps[0], "dist bound max", db.max())
    assert decided.all()                                       # the undecided share is 0 for this seed
    acc, sc = K.krum(torch.from_numpy(c.X), c.groupsize, c.n_accept)
    assert (np.abs(sc.numpy() - scores) <= sb).all()
    assert np.array_equal(acc.numpy().astype(np.int32), accept)
