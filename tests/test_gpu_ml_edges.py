"""gfx950 learning-side kernels at their batch, tile and int64 edges, against the fp64 / exact-integer references
of tests/_ml_ref.py (every case vetted on the CPU paths by tests/test_ml_ref_cpu.py).

Each group names a kernel mistake it would catch:
  softmax step   dividing the gradient by B instead of Bq = min(B, n); a K-tile loop off by one at 1024; reading
                 off / ntrain by row in resident (lo) mode
  minibatch      dropping seed >> 32 (Philox key word k1) from the draw; a duplicate index kept
  logreg step    `k += 64` written as a single pass (D > 64); dividing by Bq; calls used without % 100 in the noise
                 counter; a log-add-exp that overflows instead of saturating
  DP noise       dividing by nn = 0; iteration used without % 100; the noiser id or the seed cut to 31 / 32 bits
  recovery       a coefficient outside int64 wrapped into status 1; a division by a zero node difference; padding
                 of a strided row read into a sum; a masked-out row summed
  row sums       an out-of-range row index read; a repeated row counted once; fp64 adds out of row order
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _ml_ref as R
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu


def c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def f64(tensor):
    return tensor.cpu().numpy().astype(np.float64)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------- softmax step
@pytest.mark.parametrize("case", R.softmax_cases(), ids=lambda s: s.name)
def test_softmax_step_edges(case):
    s = case
    d_ref, l_ref = R.softmax_refs()[s.name]
    d, q, l = K.softmax_step(c(s.X), c(s.y), c(s.off), c(s.nt), c(s.pid), c(s.W), s.d_in, s.d_out, s.B, s.seed, s.it,
                             lo=s.lo)
    rtol, atol = s.tol
    print(s.name, "max |delta - ref|", np.abs(f64(d) - d_ref).max(), "max |loss - ref|", np.abs(f64(l) - l_ref).max())
    np.testing.assert_allclose(f64(d), d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(f64(l), l_ref, rtol=1e-4, atol=1e-5)
    # exact: Go's int64(float64(delta) * 10^precision) of the kernel's own delta
    np.testing.assert_array_equal(q.cpu().numpy(), np.trunc(f64(d) * R.QSCALE).astype(np.int64))


def _softmax_raw(d_in, d_out, B, ones=None, nones=0):
    n = 4
    X, y = torch.rand((n, max(d_in, 1))).cuda(), torch.zeros(n, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), i32([n]), i32([0])
    nparam = d_out * d_in + d_out
    W = torch.zeros(max(nparam, 1), dtype=torch.float64).cuda()
    delta = torch.zeros((1, max(nparam, 1)), dtype=torch.float32).cuda()
    qdelta = torch.zeros((1, max(nparam, 1)), dtype=torch.int64).cuda()
    loss = torch.zeros(1, dtype=torch.float32).cuda()
    rc = hip().bsc_softmax_step(X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(), W.data_ptr(),
                                d_in, d_out, B, 1, 7, 0, 100.0, R.QSCALE, delta.data_ptr(), qdelta.data_ptr(),
                                loss.data_ptr(), -1, None if ones is None else ones.data_ptr(), nones, stream())
    torch.cuda.synchronize()
    return rc


def test_softmax_launcher_limits_and_ones():
    assert _softmax_raw(8, 17, 4) == -1
    assert _softmax_raw(8, 4, 17) == -1
    assert _softmax_raw(0, 4, 4) == -1
    ones = torch.full((301,), -7, dtype=torch.int32).cuda()
    assert _softmax_raw(8, 4, 4, ones, 300) == 0
    assert ones.cpu().tolist() == [1] * 300 + [-7]      # more than one pass of the 256 threads; the canary stays


def _softmax_sets(n, seed):
    X, y, off, nt, pid, W = R.onehot_softmax(n)
    d = K.softmax_step(c(X), c(y), c(off), c(nt), c(pid), c(W), n, 2, 10, seed, 4)[0].cpu().numpy()
    return [R.decode_softmax(d[p], n, 10) for p in range(len(pid))], pid


@pytest.mark.parametrize("n", [3, 16, 37])
@pytest.mark.parametrize("seed", [7, 0xC0FFEE1234567890])
def test_softmax_minibatch_decoded_exactly(n, seed):
    sets, pid = _softmax_sets(n, seed)
    for p, got in enumerate(sets):
        assert got == set(K.minibatch_indices(int(pid[p]), 4, n, 10, seed)) and len(got) == min(n, 10)


def test_softmax_minibatch_reads_the_seeds_high_half():
    a, b = 0xC0FFEE1234567890, 0x00FFEE0034567890      # equal low halves
    sa, _ = _softmax_sets(37, a)
    sb, _ = _softmax_sets(37, b)
    assert any(x != y for x, y in zip(sa, sb))


# ---------------------------------------------------------------------------- logistic step
def _logreg(s, seed=None, calls=None):
    return K.logreg_step(c(s.X), c(s.y), c(s.off), c(s.nrows), c(s.pid), c(s.W), s.B, s.seed if seed is None else seed,
                         c(s.calls if calls is None else calls), s.alpha, s.lammy, c(s.sigma))


@pytest.mark.parametrize("case", R.logreg_cases(), ids=lambda s: s.name)
def test_logreg_step_edges(case):
    s = case
    ref, _ = R.logreg_refs()[s.name]
    d, q = _logreg(s)
    err = np.abs(f64(d) - ref.astype(np.float32).astype(np.float64))
    lim = R.logreg_atol(s, ref)
    print(s.name, "max err / bound", (err / lim).max())
    assert (err <= lim).all()
    quiet = s.sigma == 0
    np.testing.assert_array_equal(q.cpu().numpy()[quiet], np.trunc(ref[quiet] * R.QSCALE).astype(np.int64))
    assert (np.abs(q.cpu().numpy()[~quiet] - ref[~quiet] * R.QSCALE) <= lim[~quiet] * R.QSCALE + 1).all()


def test_logreg_saturated_residuals_are_exact():
    """lammy = 0: the gradient column of a row with y * z = +800.5 is exactly zero (residual 0), the column of a row
    with y * z = -800.5 is x * (-y) / B (residual -y)."""
    s = R.saturated_case(0.0)
    d, q = _logreg(s)
    d, q = f64(d)[0], q.cpu().numpy()[0]
    assert d[0] == 0 and d[3] == 0 and q[0] == 0 and q[3] == 0
    for k in (1, 2):
        want = -s.alpha * (s.X[k, k] * -s.y[k] / s.B)
        assert abs(d[k] - np.float32(want)) <= R.f32_ulp(want) and q[k] == int(want * R.QSCALE)


def test_logreg_launcher_rejects_B_65():
    s = R.logreg_cases()[0]
    d, q = torch.zeros((3, 1), dtype=torch.float32).cuda(), torch.zeros((3, 1), dtype=torch.int64).cuda()
    t = [c(v) for v in (s.X, s.y, s.off, s.nrows, s.pid, s.W, s.calls, s.sigma)]
    rc = hip().bsc_logreg_step(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                               t[5].data_ptr(), 1, 65, 3, s.seed, t[6].data_ptr(), s.alpha, s.lammy, t[7].data_ptr(),
                               R.QSCALE, d.data_ptr(), q.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == -1


def test_logreg_noise_wraps_at_100_calls_and_reads_the_high_key_bits():
    """X = 0 leaves the noise alone in delta: calls 205 and 5 give the same bits, seed bits 39 and 63 change them,
    bit 3 (below the noise key's shift of 7) does not."""
    D, B = 65, 10
    X, y = np.zeros((20, D)), np.ones(20)
    off, nrows, pid = np.zeros(1, np.int64), np.asarray([20], np.int32), np.asarray([4], np.int32)
    s = R.LrCase("noise", X, y, off, nrows, pid, np.zeros(D), B, R.LR_SEED, None, 1e-2, 0.0, np.asarray([0.7]))

    def run(calls, seed):
        return _logreg(s, seed, np.asarray([calls], np.int32))[0].cpu().numpy()
    base = run(205, R.LR_SEED)
    ref = R.logreg_step_ref(X, y, off, nrows, pid, s.W, B, R.LR_SEED, [205], 1e-2, 0.0, s.sigma)[0]
    assert (np.abs(base - ref.astype(np.float32)) <= R.logreg_atol(s, ref)).all()
    assert np.array_equal(base, run(5, R.LR_SEED)) and not np.array_equal(base, run(6, R.LR_SEED))
    assert not np.array_equal(base, run(205, R.LR_SEED ^ (1 << 63)))
    assert not np.array_equal(base, run(205, R.LR_SEED ^ (1 << 39)))
    assert np.array_equal(base, run(205, R.LR_SEED ^ (1 << 3)))


def _logreg_sets(n, seed):
    X, y, off, nrows, pid, W = R.onehot_logreg(n)
    calls = np.full(len(pid), 9, np.int32)
    d = K.logreg_step(c(X), c(y), c(off), c(nrows), c(pid), c(W), 10, seed, c(calls), 1e-2, 1e-2,
                      c(np.zeros(len(pid))))[0].cpu().numpy()
    return d, y, pid


@pytest.mark.parametrize("n", [3, 16, 37])
@pytest.mark.parametrize("seed", [7, 0xC0FFEE1234567890])
def test_logreg_minibatch_decoded_exactly(n, seed):
    d, y, pid = _logreg_sets(n, seed)
    for p in range(len(pid)):
        want = set(K.minibatch_indices(int(pid[p]), 9, n, 10, seed, tag=0x106))
        assert set(np.nonzero(d[p])[0].tolist()) == want
        for k in want:      # g[k] = -y / (2 B)
            assert abs(d[p, k] - np.float32(1e-2 * y[p * n + k] / 20)) <= R.f32_ulp(1e-2 / 20)


def test_logreg_minibatch_reads_the_seeds_high_half():
    da, _, pid = _logreg_sets(37, 0xC0FFEE1234567890)
    db, _, _ = _logreg_sets(37, 0x00FFEE0034567890)      # equal low halves
    assert any(set(np.nonzero(da[p])[0].tolist()) != set(np.nonzero(db[p])[0].tolist()) for p in range(len(pid)))


# ---------------------------------------------------------------------------- DP noise
@pytest.mark.parametrize("D", R.DP_DIMS)
def test_dp_noise_edges(D):
    delta, noisers, scales = R.dp_case(D)
    ref = R.dp_noise_ref(delta, noisers, scales, R.DP_SEED, 13)
    got = K.dp_noise(c(delta), c(noisers), c(scales), R.DP_SEED, 13)
    np.testing.assert_allclose(f64(got), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(got, K.dp_noise(c(delta), c(noisers), c(scales), R.DP_SEED, 113))
    hi = K.dp_noise(c(delta), c(noisers), c(scales), R.DP_SEED ^ (0x5A5A5A5A << 32), 13)
    assert (hi - got).abs().max().item() > 1e-2
    np.testing.assert_allclose(f64(hi), R.dp_noise_ref(delta, noisers, scales, R.DP_SEED ^ (0x5A5A5A5A << 32), 13),
                               rtol=1e-4, atol=1e-4)
    # no noisers, and all scales zero: the deltas themselves, bit for bit
    none = K.dp_noise(c(delta), torch.zeros((3, 0), dtype=torch.int32).cuda(), torch.zeros((3, 0)).cuda(), R.DP_SEED, 13)
    assert torch.equal(none, c(delta))
    assert torch.equal(K.dp_noise(c(delta), c(noisers), c(np.zeros_like(scales)), R.DP_SEED, 13), c(delta))


@pytest.mark.parametrize("D", R.DP_DIMS)
def test_dp_noise_table_bit_identical_at_small_D(D):
    delta, _, scales = R.dp_case(D)
    noisers = np.asarray([[0, 11], [5, 0], [11, 7]], np.int32)
    tbl = K.noise_table(12, D, R.DP_SEED, "cuda")
    for it in (13, 113, 99):
        a = K.dp_noise(c(delta), c(noisers), c(scales), R.DP_SEED, it)
        assert torch.equal(a, K.dp_noise(c(delta), c(noisers), c(scales), R.DP_SEED, it, table=tbl)), it
    np.testing.assert_allclose(f64(a), R.dp_noise_ref(delta, noisers, scales, R.DP_SEED, 99), rtol=1e-4, atol=1e-4)
    none = K.dp_noise(c(delta), torch.zeros((3, 0), dtype=torch.int32).cuda(), torch.zeros((3, 0)).cuda(), R.DP_SEED, 13,
                      table=tbl)
    assert torch.equal(none, c(delta))


# ---------------------------------------------------------------------------- recovery
@lru_cache(maxsize=None)
def _weights(xs: tuple):
    w = K.recovery_weights(list(xs), R.POLY)
    return w, c(w["A"].reshape(-1)), i32(w["basis"])


def _rows(ys, mask, cols, xs, W):
    w, A, basis = _weights(tuple(xs))
    out = K.recover_rows(c(ys), None if mask is None else i32(mask), i32(cols), i32(xs), w, A, basis, R.POLY, R.D_REC,
                         c(W))
    return [o.cpu().numpy() for o in out]


def _newton(agg, xs, W):
    return [o.cpu().numpy() for o in K.recover(c(agg), i32(xs), R.POLY, R.D_REC, c(W))]


def _recover_w_raw(ys, nrows, rstride, nch, T, mask, cols, xs, W, poly=R.POLY, h_W=None, h_status=None, wxs=None):
    """bsc_recover_w_clock called directly: (rc, W_new, coeffs, status, agg).  wxs: the layout whose weights are
    passed when xs itself is one the launcher must refuse."""
    w, A, basis = _weights(tuple(xs if wxs is None else wxs))
    Wd = c(W)
    W_new, co = torch.zeros_like(Wd), torch.zeros((nch, poly), dtype=torch.int64).cuda()
    st, agg = torch.full((nch,), -1, dtype=torch.int32).cuda(), torch.zeros((nch, len(xs)), dtype=torch.int64).cuda()
    ycols, xs_t = i32(cols), i32(xs)
    rc = hip().bsc_recover_w_clock(ys.data_ptr(), nrows, rstride, nch, T, None if mask is None else mask.data_ptr(),
                                   ycols.data_ptr(), xs_t.data_ptr(), len(xs), A.data_ptr(), basis.data_ptr(), poly,
                                   w["shift"], w["inv_lo"], w["inv_hi"], R.D_REC, Wd.data_ptr(), R.QSCALE,
                                   W_new.data_ptr(), co.data_ptr(), st.data_ptr(), agg.data_ptr(),
                                   None if h_W is None else h_W.data_ptr(),
                                   None if h_status is None else h_status.data_ptr(), None, stream())
    torch.cuda.synchronize()
    return rc, W_new, co, st, agg


@pytest.mark.parametrize("cset", R.COEFF_SETS)
@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_recover_layouts_at_the_ends_of_int64(layout, cset):
    s = R.recovery_case(layout, cset)
    want_W = R.w_expected(s.W, s.coeffs)
    Wn, co, st = _newton(s.agg, s.xs, s.W)
    assert st.tolist() == [1] * R.NCH and co.tolist() == s.coeffs
    assert np.array_equal(Wn, want_W)
    Wn, co, st, agg = _rows(s.ys, R.MASK, s.cols, s.xs, s.W)
    assert np.array_equal(agg, s.agg)
    assert st.tolist() == [1] * R.NCH and co.tolist() == s.coeffs
    assert np.array_equal(Wn, want_W)


@pytest.mark.parametrize("name,x,amount", R.tampers(), ids=[n for n, _, _ in R.tampers()])
def test_recover_rows_tampers(name, x, amount):
    s = R.recovery_case("all21", "uniform8e9")
    ys = R.tampered(s, x, amount)
    status = [0 if k in R.TAMPER_CHUNKS else 1 for k in range(R.NCH)]
    want_co = [s.coeffs[k] if status[k] else [0] * R.POLY for k in range(R.NCH)]
    want_W = R.w_expected(s.W, s.coeffs, status)
    for k in R.TAMPER_CHUNKS:       # W itself, bit for bit, on the tampered chunks
        assert np.array_equal(want_W[k * R.POLY:(k + 1) * R.POLY], s.W[k * R.POLY:(k + 1) * R.POLY])
    Wn, co, st, agg = _rows(ys, R.MASK, s.cols, s.xs, s.W)
    assert st.tolist() == status and co.tolist() == want_co and np.array_equal(Wn, want_W)
    want_agg = s.agg.copy()
    want_agg[list(R.TAMPER_CHUNKS), s.xs.index(x)] += amount
    assert np.array_equal(agg, want_agg)
    Wn, co, st = _newton(agg, s.xs, s.W)       # the 128-bit Newton kernel on the same sums
    assert st.tolist() == status and co.tolist() == want_co and np.array_equal(Wn, want_W)


def test_recover_coefficients_outside_int64(rt):
    """Shares of 61 bits whose exact coefficients are integers of up to 72 bits: no recovery, as on the host."""
    agg, expect, W = R.overflow_case()
    status = [0 if e is None else 1 for e in expect]
    want_co = [e or [0] * R.POLY for e in expect]
    want_W = R.w_expected(W, want_co)
    for k in R.TAMPER_CHUNKS:
        assert rt.recover_exact(R.OVERFLOW_XS, [int(v) for v in agg[k]], R.POLY - 1) is None
    Wn, co, st = _newton(agg, R.OVERFLOW_XS, W)
    assert st.tolist() == status and co.tolist() == want_co and np.array_equal(Wn, want_W)
    Wn, co, st, agg2 = _rows(agg[None], None, list(range(10)), R.OVERFLOW_XS, W)     # nrows = 1, no mask, T = 10
    assert np.array_equal(agg2, agg)
    assert st.tolist() == status and co.tolist() == want_co and np.array_equal(Wn, want_W)


def test_recover_repeated_x_is_no_recovery():
    """Two equal x-points among the basis nodes: status 0 on every chunk, as recover_exact returns None.  (The
    kernel divided by the zero node difference before it checked for one; the chunks ended with status 0 then
    too, so this test pins the behaviour and did not fail before the check.)"""
    xs, agg, W = R.repeated_x_case()
    Wn, co, st = _newton(agg, xs, W)
    assert not st.any() and not co.any() and np.array_equal(Wn, W)


def test_recover_launcher_limits():
    s = R.recovery_case("all21", "zero")
    xs9 = list(range(-4, 5))
    Wn, co, st = [o.cpu().numpy() for o in K.recover(c(s.agg[:, 6:15]), i32(xs9), R.POLY, R.D_REC, c(s.W))]
    assert not st.any() and not co.any() and np.array_equal(Wn, s.W)          # npts < poly: status 0 everywhere
    ys = c(s.ys)
    assert _recover_w_raw(ys, 6, R.NCH * R.T, R.NCH, R.T, None, [x + 10 for x in xs9], xs9, s.W, wxs=s.xs)[0] == -1
    xs33 = list(range(-16, 17))
    assert _recover_w_raw(ys, 6, R.NCH * R.T, R.NCH, R.T, None, [0] * 33, xs33, s.W, wxs=s.xs)[0] == -1
    assert _recover_w_raw(ys, 6, R.NCH * R.T, R.NCH, R.T, None, s.cols, s.xs, s.W, poly=17)[0] == -1
    out = [torch.zeros(R.NCH * 17, dtype=torch.int64).cuda(), torch.zeros(R.NCH, dtype=torch.int32).cuda()]
    Wd, agg33 = c(s.W), torch.zeros((R.NCH, 33), dtype=torch.int64).cuda()
    for npts, poly in ((33, R.POLY), (21, 17)):
        rc = hip().bsc_recover(agg33.data_ptr(), R.NCH, npts, i32(xs33).data_ptr(), poly, R.D_REC, Wd.data_ptr(),
                               R.QSCALE, torch.zeros_like(Wd).data_ptr(), out[0].data_ptr(), out[1].data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == -1


def test_recover_rows_masks_and_single_row():
    s = R.recovery_case("two_miners14", "uniform8e9")
    Wn, co, st, agg = _rows(s.ys, [0] * 6, s.cols, s.xs, s.W)        # nothing kept: the zero polynomial
    assert not agg.any() and not co.any() and st.tolist() == [1] * R.NCH and np.array_equal(Wn, s.W)
    tot = np.zeros((1, R.NCH, R.T), np.int64)                         # nrows = 1, no mask: ys already holds totals
    tot[0][:, s.cols] = s.agg
    Wn, co, st, agg = _rows(tot, None, s.cols, s.xs, s.W)
    assert np.array_equal(agg, s.agg) and co.tolist() == s.coeffs and st.all()
    assert np.array_equal(Wn, R.w_expected(s.W, s.coeffs))


def test_recover_rows_strided_rows_and_pinned_mirrors():
    """rstride = nch * T + 5 with the padding at 2^63 - 1 (one of them summed would show in agg), and the pinned
    h_W / h_status mirrors equal to the device outputs once the stream is synchronised."""
    s = R.recovery_case("shuffled21", "uniform8e9")
    R6, stride = len(R.MASK), R.NCH * R.T + 5
    buf = np.full((R6, stride), R.I64_MAX, np.int64)
    buf[:, : R.NCH * R.T] = s.ys.reshape(R6, -1)
    h_W = torch.full((R.D_REC,), float("nan"), dtype=torch.float64).pin_memory()
    h_st = torch.full((R.NCH,), -1, dtype=torch.int32).pin_memory()
    rc, Wn, co, st, agg = _recover_w_raw(c(buf), R6, stride, R.NCH, R.T, i32(R.MASK), s.cols, s.xs, s.W, h_W=h_W,
                                         h_status=h_st)
    assert rc == 0
    assert np.array_equal(agg.cpu().numpy(), s.agg)
    assert st.cpu().tolist() == [1] * R.NCH and co.cpu().numpy().tolist() == s.coeffs
    assert np.array_equal(Wn.cpu().numpy(), R.w_expected(s.W, s.coeffs))
    assert torch.equal(h_W, Wn.cpu()) and torch.equal(h_st, st.cpu())


# ---------------------------------------------------------------------------- row sums
@pytest.mark.parametrize("C", [1, 257])
def test_sum_rows_i64_edges(C):
    g = np.random.default_rng(C)
    ys = (2 ** 60 - g.integers(0, 1000, (6, C))) * g.choice([-1, 1], (6, C))
    big = ys.astype(object)
    rows = [-1, 6, 2, 2, 0, 5]          # below 0 and >= R: skipped; 2 counted twice
    got = K.sum_rows_i64(c(ys), rows=i32(rows)).cpu().numpy()
    assert got.tolist() == (2 * big[2] + big[0] + big[5]).tolist()
    mask = [1, 0, 1, 1, 0, 0]
    got = K.sum_rows_i64(c(ys), rows=i32(rows), mask=i32(mask)).cpu().numpy()
    assert got.tolist() == (2 * big[2] + big[0]).tolist()
    assert K.sum_rows_i64(c(ys), mask=i32(mask)).cpu().numpy().tolist() == (big[0] + big[2] + big[3]).tolist()
    assert K.sum_rows_i64(c(ys)).cpu().numpy().tolist() == big.sum(0).tolist()


@pytest.mark.parametrize("D", [1, 257])
def test_add_rows_edges(D):
    g = np.random.default_rng(D)
    delta = g.standard_normal((5, D)).astype(np.float32)
    W = g.standard_normal(D)
    rows = [3, 3, 0, 4, 3]
    want = W.copy()
    for r in rows:      # sequential fp64 adds in row order
        want = want + delta[r].astype(np.float64)
    assert np.array_equal(K.add_rows(c(delta), i32(rows), c(W)).cpu().numpy(), want)
    none = K.add_rows(c(delta), torch.zeros(0, dtype=torch.int32).cuda(), c(W))
    assert np.array_equal(none.cpu().numpy(), W)
