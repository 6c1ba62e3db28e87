"""The learning-kernel edge cases (tests/_ml_ref.py) against the project's CPU paths, at the tolerances the GPU
tests use: every input set is vetted here before it reaches a kernel.  No GPU."""
import numpy as np
import pytest
import torch

import _ml_ref as R
from biscotti_amd.ops import ml as K

t = torch.from_numpy


# ---------------------------------------------------------------------------- softmax step
@pytest.mark.parametrize("case", R.softmax_cases(), ids=lambda c: c.name)
def test_softmax_cpu_path_matches_reference(case):
    c = case
    d_ref, l_ref = R.softmax_refs()[c.name]
    d, q, l = K.softmax_step(t(c.X), t(c.y), t(c.off), t(c.nt), t(c.pid), t(c.W), c.d_in, c.d_out, c.B, c.seed, c.it,
                             lo=c.lo)
    rtol, atol = c.tol
    np.testing.assert_allclose(d.numpy().astype(np.float64), d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l.numpy().astype(np.float64), l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.numpy(), np.trunc(d.numpy().astype(np.float64) * R.QSCALE).astype(np.int64))
    assert np.isfinite(d_ref).all() and np.abs(d_ref).max() > 1e-3      # the case says something


@pytest.mark.parametrize("n", [3, 16, 37])
@pytest.mark.parametrize("seed", [7, 0xC0FFEE1234567890])
def test_softmax_onehot_decodes_the_minibatch(n, seed):
    X, y, off, nt, pid, W = R.onehot_softmax(n)
    for ref in (True, False):
        d = (R.softmax_step_ref(X, y, off, nt, pid, W, n, 2, 10, seed, 4)[0] if ref else
             K.softmax_step(t(X), t(y), t(off), t(nt), t(pid), t(W), n, 2, 10, seed, 4)[0].numpy())
        for p in range(len(pid)):
            assert R.decode_softmax(d[p], n, 10) == set(K.minibatch_indices(int(pid[p]), 4, n, 10, seed))


def test_minibatch_depends_on_the_seeds_high_half():
    a, b = 0xC0FFEE1234567890, 0x00FFEE0034567890
    assert a & R.M32 == b & R.M32
    assert any(set(K.minibatch_indices(p * 5 + 1, 4, 37, 10, a)) != set(K.minibatch_indices(p * 5 + 1, 4, 37, 10, b))
               for p in range(8))
    assert any(set(K.minibatch_indices(p * 3 + 2, 9, 37, 10, a, tag=0x106))
               != set(K.minibatch_indices(p * 3 + 2, 9, 37, 10, b, tag=0x106)) for p in range(8))


# ---------------------------------------------------------------------------- logistic step
@pytest.mark.filterwarnings("ignore:overflow encountered in exp")      # the saturated rows, on purpose
@pytest.mark.parametrize("case", R.logreg_cases(), ids=lambda c: c.name)
def test_logreg_cpu_path_matches_reference(case):
    c = case
    ref, _ = R.logreg_refs()[c.name]
    d, q = K.logreg_step(t(c.X), t(c.y), t(c.off), t(c.nrows), t(c.pid), t(c.W), c.B, c.seed, t(c.calls), c.alpha,
                         c.lammy, t(c.sigma))
    err = np.abs(d.numpy().astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    assert (err <= R.logreg_atol(c, ref)).all(), err.max()
    quiet = c.sigma == 0
    # the condition of the exact qdelta check: no reference value within 1e-6 of a truncation boundary
    s = ref[quiet] * R.QSCALE
    assert np.abs(s - np.rint(s)).min() > 1e-6
    np.testing.assert_array_equal(q.numpy()[quiet], np.trunc(s).astype(np.int64))
    noisy = ~quiet
    lim = R.logreg_atol(c, ref)[noisy] * R.QSCALE + 1
    assert (np.abs(q.numpy()[noisy] - ref[noisy] * R.QSCALE) <= lim).all()


def test_logreg_saturated_branches_in_the_reference():
    """The residual is exactly 0 where y * z = +800.5 and exactly -y where it is -800.5."""
    for lammy in (0.01, 0.0):
        c = R.saturated_case(lammy)
        _, res = R.logreg_step_ref(c.X, c.y, c.off, c.nrows, c.pid, c.W, c.B, c.seed, c.calls, c.alpha, c.lammy, c.sigma)
        idx = K.minibatch_indices(int(c.pid[0]), int(c.calls[0]), 4, 4, c.seed, tag=0x106)
        assert sorted(idx) == [0, 1, 2, 3]
        for s, row in enumerate(idx):
            tz = c.y[row] * c.X[row, row]
            assert abs(tz) == 800.5
            assert res[0][s] == (0.0 if tz > 0 else -c.y[row])


def test_logreg_noise_wraps_at_100_calls_and_reads_the_high_key_bits():
    """X = 0 leaves the noise alone in delta: calls 205 and 5 agree, seed bits 39 and 63 change it, bit 3 does not."""
    D, B = 65, 10
    X, y = np.zeros((20, D)), np.ones(20)
    off, nrows, pid = np.zeros(1, np.int64), np.asarray([20], np.int32), np.asarray([4], np.int32)
    W, sigma = np.zeros(D), np.asarray([0.7])

    def run(calls, seed):
        ref = R.logreg_step_ref(X, y, off, nrows, pid, W, B, seed, [calls], 1e-2, 0.0, sigma)[0]
        got = K.logreg_step(t(X), t(y), t(off), t(nrows), t(pid), t(W), B, seed, torch.tensor([calls], dtype=torch.int32),
                            1e-2, 0.0, t(sigma))[0].numpy()
        c = R.LrCase("", X, y, off, nrows, pid, W, B, seed, None, 1e-2, 0.0, sigma)
        assert (np.abs(got - ref.astype(np.float32)) <= R.logreg_atol(c, ref)).all()
        return ref
    base = run(205, R.LR_SEED)
    assert np.array_equal(base, run(5, R.LR_SEED)) and not np.array_equal(base, run(6, R.LR_SEED))
    assert not np.array_equal(base, run(205, R.LR_SEED ^ (1 << 63)))
    assert not np.array_equal(base, run(205, R.LR_SEED ^ (1 << 39)))
    assert np.array_equal(base, run(205, R.LR_SEED ^ (1 << 3)))


@pytest.mark.parametrize("n", [3, 16, 37])
@pytest.mark.parametrize("seed", [7, 0xC0FFEE1234567890])
def test_logreg_onehot_decodes_the_minibatch(n, seed):
    X, y, off, nrows, pid, W = R.onehot_logreg(n)
    calls = np.full(len(pid), 9, np.int32)
    d = K.logreg_step(t(X), t(y), t(off), t(nrows), t(pid), t(W), 10, seed, t(calls), 1e-2, 1e-2,
                      t(np.zeros(len(pid))))[0].numpy()
    ref = R.logreg_step_ref(X, y, off, nrows, pid, W, 10, seed, calls, 1e-2, 1e-2, np.zeros(len(pid)))[0]
    for p in range(len(pid)):
        want = set(K.minibatch_indices(int(pid[p]), 9, n, 10, seed, tag=0x106))
        assert set(np.nonzero(d[p])[0].tolist()) == want == set(np.nonzero(ref[p])[0].tolist())
        for k in want:
            assert abs(ref[p, k] - 1e-2 * y[p * n + k] / 20) < 1e-15


# ---------------------------------------------------------------------------- DP noise
@pytest.mark.parametrize("D", R.DP_DIMS)
def test_dp_noise_cpu_path_matches_reference(D):
    delta, noisers, scales = R.dp_case(D)
    ref = R.dp_noise_ref(delta, noisers, scales, R.DP_SEED, 13)
    got = K.dp_noise(t(delta), t(noisers), t(scales), R.DP_SEED, 13).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    assert np.array_equal(ref, R.dp_noise_ref(delta, noisers, scales, R.DP_SEED, 113))
    assert np.array_equal(got, K.dp_noise(t(delta), t(noisers), t(scales), R.DP_SEED, 113).numpy())
    hi = R.dp_noise_ref(delta, noisers, scales, R.DP_SEED ^ (0x5A5A5A5A << 32), 13)
    assert np.abs(hi - ref).max() > 1e-2
    # no noisers, and all scales zero: the deltas themselves
    assert np.array_equal(R.dp_noise_ref(delta, np.zeros((3, 0), np.int32), np.zeros((3, 0), np.float32), R.DP_SEED, 13),
                          delta.astype(np.float64))
    assert np.array_equal(K.dp_noise(t(delta), torch.zeros((3, 0), dtype=torch.int32), torch.zeros((3, 0)),
                                     R.DP_SEED, 13).numpy(), delta)
    assert np.array_equal(K.dp_noise(t(delta), t(noisers), t(np.zeros_like(scales)), R.DP_SEED, 13).numpy(), delta)


# ---------------------------------------------------------------------------- recovery
def _cpu_recover(agg, xs, W):
    Wn, co, st = K.recover(t(np.ascontiguousarray(agg)), torch.tensor(xs, dtype=torch.int32), R.POLY, R.D_REC, t(W))
    return Wn.numpy(), co.numpy(), st.numpy()


@pytest.mark.parametrize("cset", R.COEFF_SETS)
@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_recovery_cpu_paths_match_reference(layout, cset, rt):
    c = R.recovery_case(layout, cset)
    # every share and every partial sum over the kept rows, in row order, fits int64
    kept = [r for r in range(len(R.MASK)) if R.MASK[r]]
    part = np.zeros(c.ys.shape[1:], dtype=object)
    for r in kept:
        part = part + c.ys[r].astype(object)
        assert all(R.I64_MIN <= int(v) <= R.I64_MAX for v in part.reshape(-1))
    np.testing.assert_array_equal(part[:, c.cols].astype(np.int64), c.agg)
    for k in range(R.NCH):
        assert R.recover_ref(c.xs, c.agg[k], R.POLY) == c.coeffs[k]
        assert rt.recover_exact(c.xs, [int(v) for v in c.agg[k]], R.POLY - 1) == c.coeffs[k]
    Wn, co, st = _cpu_recover(c.agg, c.xs, c.W)
    assert st.all()
    assert co.tolist() == c.coeffs
    assert np.array_equal(Wn, R.w_expected(c.W, c.coeffs))
    Wn2, co2, st2, agg2 = K.recover_rows(t(c.ys), torch.tensor(R.MASK, dtype=torch.int32),
                                         torch.tensor(c.cols, dtype=torch.int32), torch.tensor(c.xs, dtype=torch.int32),
                                         None, None, None, R.POLY, R.D_REC, t(c.W))
    assert np.array_equal(agg2.numpy(), c.agg) and st2.numpy().all() and co2.numpy().tolist() == c.coeffs
    assert np.array_equal(Wn2.numpy(), Wn)
    if cset == "uniform8e9" and layout == "all21":
        assert max(abs(int(v)) for v in c.agg.reshape(-1)) > 0.96 * 2 ** 63


def test_recovery_weights_denominator_matches_reference():
    for xs in R.LAYOUTS.values():
        order = R.basis_order(xs, R.POLY)
        A, Dn = R.inverse_vandermonde(tuple(xs[i] for i in order))
        w = K.recovery_weights(xs, R.POLY)
        assert w["Dn"] == Dn and w["basis"] == order and w["A"].tolist() == A


@pytest.mark.parametrize("name,x,amount", R.tampers(), ids=[n for n, _, _ in R.tampers()])
def test_recovery_tampers_on_the_cpu_paths(name, x, amount, rt):
    c = R.recovery_case("all21", "uniform8e9")
    assert (x in [c.xs[i] for i in R.basis_order(c.xs, R.POLY)]) == name.startswith("basis")
    ys = R.tampered(c, x, amount)
    agg = ys[np.asarray(R.MASK, bool)].sum(0)[:, c.cols]
    status = [0 if k in R.TAMPER_CHUNKS else 1 for k in range(R.NCH)]
    for k in range(R.NCH):
        want = None if k in R.TAMPER_CHUNKS else c.coeffs[k]
        assert R.recover_ref(c.xs, agg[k], R.POLY) == want
        assert rt.recover_exact(c.xs, [int(v) for v in agg[k]], R.POLY - 1) == want
    if "Dn" in name:   # the division stays exact: the rational solution is integral, only a share is off
        assert all(v.denominator == 1 for v in R.solve_exact(c.xs, agg[R.TAMPER_CHUNKS[0]], R.POLY))
    Wn, co, st = _cpu_recover(agg, c.xs, c.W)
    assert st.tolist() == status
    assert np.array_equal(Wn, R.w_expected(c.W, c.coeffs, status))
    assert all(co[k].tolist() == ([0] * R.POLY if k in R.TAMPER_CHUNKS else c.coeffs[k]) for k in range(R.NCH))


def test_recovery_out_of_int64_example(rt):
    agg, expect, W = R.overflow_case()
    k = R.TAMPER_CHUNKS[0]
    assert max(abs(int(v)).bit_length() for v in agg[k]) <= 61
    sol = R.solve_exact(R.OVERFLOW_XS, agg[k], R.POLY)
    assert all(v.denominator == 1 for v in sol)
    bits = [abs(int(v)).bit_length() for v in sol]
    assert min(bits) >= 51 and 64 <= max(bits) <= 72
    for k in range(R.NCH):
        assert R.recover_ref(R.OVERFLOW_XS, agg[k], R.POLY) == expect[k]
        assert rt.recover_exact(R.OVERFLOW_XS, [int(v) for v in agg[k]], R.POLY - 1) == expect[k]
    Wn, co, st = _cpu_recover(agg, R.OVERFLOW_XS, W)
    assert st.tolist() == [0 if e is None else 1 for e in expect]
    assert np.array_equal(Wn, R.w_expected(W, [e or [0] * R.POLY for e in expect]))


def test_recovery_repeated_x(rt):
    xs, agg, W = R.repeated_x_case()
    assert len(set(xs[i] for i in R.basis_order(xs, R.POLY))) < R.POLY
    for k in range(R.NCH):
        assert R.recover_ref(xs, agg[k], R.POLY) is None
        assert rt.recover_exact(xs, [int(v) for v in agg[k]], R.POLY - 1) is None
    Wn, co, st = _cpu_recover(agg, xs, W)
    assert not st.any() and not co.any() and np.array_equal(Wn, W)
