"""Single-verifier Multi-Krum (K5a-c: k_gram_f64, k_krum_scores, k_krum_accept) and the LSH sieve kernels (LS1-LS3:
k_lsh_codes, k_lsh_count, k_weighted_rows) at their tile, split, window and tie edges, against the exact-integer /
fsum references of tests/_defence_ref.py (every case vetted on the CPU by tests/test_defence_ref_cpu.py).

Integer inputs make every product and partial sum representable, so distances, scores, accept flags, codes and
counts are compared with EQUALITY.  Each group names a kernel mistake it would catch:
  Gram          a tail k-step read past its split (`kx < k1`), the 32-wide loop and the 4-wide tail out of step, a
                partial 16-row tile's clamped rows leaking into the sums, rows read past the end of X (the input
                sits in front of a poisoned guard region)
  scores        the rank window [1, groupsize-1) off by one at either end, ties not ranked by column index, a
                negative rounded distance taken for rank 0's self-distance
  accept        n_accept of 0 or > n, equal scores not resolved by row index
  launcher      n > 128, D <= 0 or ksplit <= 0 doing anything but return -1
  LSH codes     `> 0` written `>= 0`, bit 31 lost, lanes without a column (D < 256) or a fourth pass (D = 600)
  LSH count     `d2 < thr` written `<=`, rows[] ignored, gram_at's tile swap, a second (partial) block of rows, a
                collision in the last table missed
  weighted rows a column past 256 dropped, rows summed out of order (exact inputs) or in less than fp64
"""
import numpy as np
import pytest
import torch

import _defence_ref as R
from biscotti_amd.native import hip
from biscotti_amd.ops import lsh
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu

GUARD = 64            # poisoned floats behind X: a read past the last row stays inside the allocation and shows
POISON = 2.0 ** 60
SENT = -7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(X):
    """(buffer, view): X [n, D] on the GPU with GUARD poisoned floats behind it in the same allocation."""
    n, D = X.shape
    buf = torch.full((n * D + GUARD,), POISON, dtype=torch.float32, device="cuda")
    buf[:n * D] = dev(X).reshape(-1)
    return buf, buf[:n * D].view(n, D)


def krum_raw(X, groupsize, n_accept, ksplit, n=None, D=None):
    """bsc_krum on sentinel-filled part / dist / scores / accept: (rc, dist, scores, accept, part) as numpy."""
    rows, cols = X.shape
    n = rows if n is None else n
    D = cols if D is None else D
    buf, Xd = guarded(X)
    na = max(rows, 1)
    npad = 16 * ((na + 15) // 16)
    nsplit = max(1, -(-max(cols, 1) // max(ksplit, 1)))
    nan = float("nan")
    part = torch.full((nsplit, npad, npad), nan, dtype=torch.float64, device="cuda")
    dist = torch.full((na, na), nan, dtype=torch.float64, device="cuda")
    scores = torch.full((na,), nan, dtype=torch.float64, device="cuda")
    acc = torch.full((na,), SENT, dtype=torch.int32, device="cuda")
    rc = hip().bsc_krum(Xd.data_ptr(), n, D, ksplit, part.data_ptr(), dist.data_ptr(), scores.data_ptr(),
                        acc.data_ptr(), groupsize, n_accept, stream())
    torch.cuda.synchronize()
    assert bool((buf[rows * cols:] == POISON).all())
    return rc, dist.cpu().numpy(), scores.cpu().numpy(), acc.cpu().numpy(), part.cpu().numpy()


def check_krum_exact(case, ref):
    d_ref, s_ref, a_ref = ref
    rc, dist, scores, acc, _ = krum_raw(case.X, case.groupsize, case.n_accept, case.ksplit)
    assert rc == 0
    # every entry overwritten: no sentinel survives, whatever sat in part's padded rows and columns
    assert not np.isnan(dist).any() and not np.isnan(scores).any() and set(acc.tolist()) <= {0, 1}
    assert np.array_equal(dist, dist.T) and not np.diag(dist).any()
    bad = np.argwhere(dist != d_ref.astype(np.float64))
    assert bad.size == 0, (case.name, "dist", bad[:5].tolist())
    assert np.array_equal(scores, s_ref.astype(np.float64)), (case.name, scores.tolist(), s_ref.tolist())
    assert np.array_equal(acc, a_ref), (case.name, acc.tolist(), a_ref.tolist())


# ---------------------------------------------------------------------------- Krum, exact
@pytest.mark.parametrize("case", R.krum_shape_cases(), ids=lambda c: c.name)
def test_krum_shapes_exact(case):
    check_krum_exact(case, R.krum_refs()[case.name])


@pytest.mark.parametrize("case", R.krum_ksplit_cases(), ids=lambda c: c.name)
def test_krum_ksplit_exact(case):
    check_krum_exact(case, R.krum_refs()[case.name])


@pytest.mark.parametrize("case", R.krum_window_cases(), ids=lambda c: c.name)
def test_krum_groupsize_and_n_accept_exact(case):
    check_krum_exact(case, R.krum_refs()[case.name])


@pytest.mark.parametrize("case", R.krum_tie_cases(), ids=lambda c: c.name)
def test_krum_ties_exact(case):
    check_krum_exact(case, R.krum_refs()[case.name])
    if case.name.startswith("identical"):
        _, _, scores, acc, _ = krum_raw(case.X, case.groupsize, case.n_accept, case.ksplit)
        assert not scores.any()
        assert acc.tolist() == [1] * min(case.n_accept, 17) + [0] * (17 - min(case.n_accept, 17))


def test_krum_padded_partials_are_zero_and_unread():
    """n = 17 fills one row and one column of the second 16-tile: the rest of part's padding is written as 0."""
    case = R.krum_ksplit_cases()[3]                            # ksplit 36: 8 splits
    rc, dist, _, _, part = krum_raw(case.X, case.groupsize, case.n_accept, case.ksplit)
    assert rc == 0 and part.shape == (8, 32, 32) and not np.isnan(part).any()
    assert not part[:, 17:, :].any() and not part[:, :, 17:].any()
    assert np.array_equal(part.sum(0)[:17, :17], R.gram_int(case.X).astype(np.float64))


def test_krum_rounded_negative_distance_keeps_rank_zero_out():
    """2^56 + q q' does not fit fp64: the (correctly rounded) Gram makes D_ij = -32 for two pairs.  Rank 0 of such a
    row is the negative entry, and the self-distance 0 at rank 1 is kept."""
    case = R.krum_rounded_case()
    d_ref, s_ref, a_ref = R.krum_ref_rounded(case.X, case.groupsize, case.n_accept)
    rc, dist, scores, acc, _ = krum_raw(case.X, case.groupsize, case.n_accept, case.ksplit)
    assert rc == 0 and dist[1, 2] == -32.0
    assert np.array_equal(dist, d_ref) and np.array_equal(scores, s_ref) and np.array_equal(acc, a_ref)


@pytest.mark.parametrize("name", ["n1_D1", "n17_D257", "n128_D31", "g19_a22", "g2_a0", "duplicates", "symmetric"])
def test_krum_through_ops(name):
    case = {c.name: c for c in R.krum_int_cases()}[name]
    _, s_ref, a_ref = R.krum_refs()[name]
    acc, sc = K.krum(dev(case.X), case.groupsize, case.n_accept, case.ksplit)
    assert acc.dtype == torch.bool and acc.device.type == "cpu"
    assert np.array_equal(sc.cpu().numpy(), s_ref.astype(np.float64))
    assert np.array_equal(acc.numpy().astype(np.int32), a_ref)


# ---------------------------------------------------------------------------- Krum, real-valued
def test_krum_real_within_gram_bound():
    case = R.krum_real_case()
    d_ref, s_ref, a_ref, db, sb, decided = R.krum_real_ref()
    rc, dist, scores, acc, _ = krum_raw(case.X, case.groupsize, case.n_accept, case.ksplit)
    assert rc == 0
    print("max |dist - ref| / bound", (np.abs(dist - d_ref) / np.where(db > 0, db, 1)).max(),
          "max |score - ref| / bound", (np.abs(scores - s_ref) / sb).max())
    assert (np.abs(dist - d_ref) <= db).all() and not np.diag(dist).any()
    assert (np.abs(scores - s_ref) <= sb).all()
    assert decided.all()                                       # no row left undecided for this seed
    assert np.array_equal(acc[decided], a_ref[decided])


# ---------------------------------------------------------------------------- Krum launcher contract
@pytest.mark.parametrize("n,D,ksplit,rows,cols", [
    (129, 4, 256, 129, 4), (17, 0, 256, 17, 4), (17, -1, 256, 17, 4), (17, 33, 0, 17, 33), (17, 33, -3, 17, 33),
    (1, 0, 0, 1, 1)])
def test_krum_launcher_rejects(n, D, ksplit, rows, cols):
    X = R._ix("reject", rows, cols)
    rc, dist, scores, acc, part = krum_raw(X, 5, 3, ksplit, n=n, D=D)
    assert rc == -1
    assert np.isnan(dist).all() and np.isnan(scores).all() and np.isnan(part).all() and (acc == SENT).all()


@pytest.mark.parametrize("n", [0, -1])
def test_krum_launcher_no_rows_is_a_noop(n):
    rc, dist, scores, acc, part = krum_raw(R._ix("noop", 3, 4), 5, 3, 256, n=n)
    assert rc == 0
    assert np.isnan(dist).all() and np.isnan(scores).all() and np.isnan(part).all() and (acc == SENT).all()
    assert K.krum(torch.empty((0, 5), device="cuda"), 3, 1)[0].numel() == 0


def test_krum_async_rejects_bad_split_and_width():
    X = dev(R._ix("async", 5, 8))
    for ksplit in (0, -1):
        with pytest.raises(ValueError, match="ksplit"):
            K.krum_async(X, 3, 2, ksplit)
    with pytest.raises(ValueError, match="D = 0"):
        K.krum_async(torch.empty((3, 0), dtype=torch.float32, device="cuda"), 3, 2)
    with pytest.raises(AssertionError):
        K.krum_async(dev(R._ix("async129", 129, 2)), 3, 2)


# ---------------------------------------------------------------------------- LSH codes (LS1)
def gpu_codes(c):
    out = lsh.codes(dev(c.X), dev(c.mu), dev(c.planes), c.L, c.K)
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(c.X), c.L)
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", R.lsh_codes_cases(), ids=lambda c: c.name)
def test_lsh_codes_exact(case):
    want = R.lsh_codes_ref(case.X, case.mu, case.planes, case.L, case.K)
    got = gpu_codes(case)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert not got[0].any()                                    # the row equal to mu


@pytest.mark.parametrize("planted", R.lsh_codes_planted(), ids=lambda p: p[0].name)
def test_lsh_codes_planted_rows(planted):
    case, want = planted
    assert np.array_equal(gpu_codes(case), want)


def codes_raw(n, D, L, K_):
    X = dev(R._ix("codes_raw", max(n, 1), D))
    mu = torch.zeros(D, dtype=torch.float32, device="cuda")
    P = torch.ones((max(L * K_, 1), D), dtype=torch.float32, device="cuda")
    out = torch.full((max(n, 1), max(L, 1)), SENT, dtype=torch.int32, device="cuda")
    rc = hip().bsc_lsh_codes(X.data_ptr(), mu.data_ptr(), n, D, P.data_ptr(), L, K_, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("n,L,K_,rc_want", [(3, 5, 13, -1), (3, 1, 33, -1), (3, 2, 0, -1), (3, 2, -1, -1),
                                            (3, 0, 12, 0), (0, 4, 12, 0)])
def test_lsh_codes_launcher_limits(n, L, K_, rc_want):
    rc, out = codes_raw(n, 7, L, K_)
    assert rc == rc_want and (out == SENT).all()


def test_lsh_codes_launcher_at_the_limits():
    for L, K_ in ((2, 32), (64, 1), (1, 32)):
        rc, out = codes_raw(3, 7, L, K_)
        assert rc == 0 and (out != SENT).all()


# ---------------------------------------------------------------------------- LSH count (LS2)
def count_raw(c, m=None):
    Xc = dev(c.X)
    pre = K.gram_stacked_async(Xc, Xc[:0])
    U = len(c.X)
    cd = dev(c.codes.view(np.int32)) if c.L else torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = torch.tensor(c.rows, dtype=torch.int32).cuda()
    m = len(c.rows) if m is None else m
    out = torch.full((len(c.rows),), SENT, dtype=torch.int32, device="cuda")
    rc = hip().bsc_lsh_count(pre["gram"].data_ptr(), U, cd.data_ptr(), c.L, rows.data_ptr(), m, float(c.thr),
                             out.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("case", R.lsh_count_cases(), ids=lambda c: c.name)
def test_lsh_count_exact(case):
    want = R.lsh_count_ref(R.gram_int(case.X), case.codes, case.L, case.rows, case.thr)
    rc, got = count_raw(case)
    assert rc == 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("planted", R.lsh_count_planted(), ids=lambda p: p[0].name)
def test_lsh_count_planted_pairs(planted):
    case, want = planted
    rc, got = count_raw(case)
    assert rc == 0 and np.array_equal(got, want)
    assert np.array_equal(want, R.lsh_count_ref(R.gram_int(case.X), case.codes, case.L, case.rows, case.thr))


def test_lsh_count_no_rows_writes_nothing():
    case = R.lsh_count_cases()[2]
    for m in (0, -1):
        rc, got = count_raw(case, m=m)
        assert rc == 0 and (got == SENT).all()


@pytest.mark.parametrize("case", R.sieve_cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("tables", [0, 4])
def test_lsh_neighbour_counts_and_sieve_accept(case, tables):
    Xc = dev(case.X)
    inboxes = [list(r) for r in case.inboxes]
    G = R.gram_int(case.X)
    cd = None
    if tables:
        P = lsh.planes(tables, 6, Xc.shape[1], 11, Xc.device)
        cd = lsh.codes(Xc, Xc.mean(0), P, tables, 6).cpu().numpy()
    got = lsh.neighbour_counts(Xc, case.thr, inboxes, tables=tables, bits=6, seed=11)
    assert len(got) == 2
    for rows, g in zip(case.inboxes, got):
        want = R.lsh_count_ref(G, cd, tables, rows, case.thr)
        assert g.tolist() == want.tolist()
        assert want.max() > 1
    d = Xc.shape[1]
    for rows in case.inboxes:                                  # (sieve_accept stacks: one inbox length per call)
        acc = lsh.sieve_accept(Xc, [list(rows)], d, tables=tables, bits=6, seed=11)
        want = R.lsh_count_ref(G, cd, tables, rows, 1.0 / d) == 1
        assert acc.shape == (1, len(rows)) and acc[0].tolist() == want.tolist() and want.any() and not want.all()


# ---------------------------------------------------------------------------- weighted rows (LS3)
def weighted_raw(X, w):
    n, D = X.shape
    Xc, wc = dev(X), dev(np.asarray(w, np.float64))
    out = torch.full((D,), float("nan"), dtype=torch.float64, device="cuda")
    rc = hip().bsc_weighted_rows(Xc.data_ptr(), n, D, wc.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("case", R.weighted_int_cases(), ids=lambda c: c.name)
def test_weighted_rows_exact(case):
    w = 1.0 / case.cnt.astype(np.float64)
    assert np.array_equal(weighted_raw(case.X, w), R.weighted_rows_ref(case.X, w))


def test_weighted_rows_real_within_bound():
    case = R.weighted_real_case()
    w = 1.0 / case.cnt.astype(np.float64)
    got, ref, bound = weighted_raw(case.X, w), R.weighted_rows_ref(case.X, w), R.weighted_rows_bound(case.X, w)
    print("max |out - ref| / bound", (np.abs(got - ref) / bound).max())
    assert (np.abs(got - ref) <= bound).all()


def test_lsh_sieve_on_the_sybil_sample():
    from test_lsh import _sample
    X = torch.from_numpy(_sample()).float()
    grad, cnt = lsh.lsh_sieve(X.cuda(), tables=0)
    assert (cnt[-10:] == 10).all() and (cnt[:50] >= 1).all()
    w = 1.0 / cnt.double().numpy()
    ref, bound = R.weighted_rows_ref(X.numpy(), w), R.weighted_rows_bound(X.numpy(), w)
    assert grad.dtype == torch.float64 and (np.abs(grad.cpu().numpy() - ref) <= bound).all()
