"""Committee RONI off the GPU: the accept rule, the CPU form of the batched op (the existing eval_error looped over
the same rows and models), the minibatch rows the task hands the kernel, and the CPU engine, which keeps the
per-candidate loop."""
import numpy as np
import torch

from biscotti_amd import data as D
from biscotti_amd.models.tasks import SoftmaxTask
from biscotti_amd.ops import ml as K
from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine


def test_roni_accept_hand_written_counts():
    counts = np.array([[3, 3, 4, 0, 10],     # 10 rows: base 3 errors
                       [1, 1, 2, 0, 4]],     # 4 rows: base 1 error
                      np.uint32)
    ok = K.roni_accept(counts, np.array([10, 4], np.int32))
    assert ok.dtype == bool and ok.shape == (2, 4)
    assert ok.tolist() == [[True, False, True, False], [True, False, True, False]]
    # the loop's own arithmetic: train_error(W + u) - train_error(W) <= 0.02 on Python floats
    for v, n in enumerate((10, 4)):
        for j in range(4):
            assert ok[v, j] == (int(counts[v, 1 + j]) / n - int(counts[v, 0]) / n <= 0.02)


def test_roni_accept_boundary_batch_of_ten():
    """B = 10: one more error than the base model is +0.1 > 0.02 (rejected); as many or fewer are accepted."""
    for base in range(0, 10):
        counts = np.array([[base] + list(range(0, 11))], np.uint32)
        ok = K.roni_accept(counts, np.array([10], np.int32))[0]
        assert ok.tolist() == [c <= base for c in range(0, 11)], base


def test_roni_accept_boundary_hundred_rows():
    """nrows = 100: +2 errors (0.02) passes, +3 does not -- the only size where the rule is not 'no worse'."""
    for base in (0, 7, 50, 97):
        counts = np.array([[base, base, base + 1, base + 2, base + 3]], np.uint32)
        ok = K.roni_accept(counts, np.array([100], np.int32))[0]
        assert ok.tolist() == [True, True, (base + 2) / 100 - base / 100 <= 0.02, False], base
    # 2/100 - 0/100 is 0.02 exactly; for other bases the float64 difference decides, as it does in the loop
    assert K.roni_accept(np.array([[0, 2]], np.uint32), np.array([100], np.int32))[0, 0]
    assert K.roni_accept(np.array([[0, 2]], np.uint32), np.array([100], np.int32), threshold=0.019)[0, 0] == False  # noqa: E712


def _inputs(d_in, d_out, V, ni, B, seed=0, n_rows=97, n_cand=None):
    g = torch.Generator().manual_seed(seed)
    n_cand = n_cand or ni + 3
    X = torch.rand((n_rows, d_in), generator=g, dtype=torch.float32)
    y = torch.randint(0, d_out, (n_rows,), generator=g, dtype=torch.int32)
    W = torch.randn((d_out * d_in + d_out,), generator=g, dtype=torch.float64)
    U = 0.1 * torch.randn((n_cand, d_out * d_in + d_out), generator=g, dtype=torch.float32)
    rows = torch.stack([torch.randperm(n_rows, generator=g)[:B] for _ in range(V)]).to(torch.int64)
    nrows = torch.full((V,), B, dtype=torch.int32)
    cand = torch.stack([torch.randperm(n_cand, generator=g)[:ni] for _ in range(V)]).to(torch.int32)
    return X, y, W, U, rows, nrows, cand


def test_roni_committee_cpu_equals_eval_error_loop():
    d_in, d_out, V, ni, B = 70, 3, 2, 5, 10
    X, y, W, U, rows, nrows, cand = _inputs(d_in, d_out, V, ni, B)
    nrows[1] = 7   # a short minibatch: the padded slots are never counted
    got = K.roni_committee(X, y, rows, nrows, W, U, cand, d_in, d_out)
    assert got.shape == (V, ni + 1) and got.dtype == np.uint32
    want = np.zeros((V, ni + 1), np.int64)
    for v in range(V):
        n = int(nrows[v])
        sel = rows[v, :n]
        models = [W] + [W + U[int(c)].double() for c in cand[v]]
        for j, Wm in enumerate(models):
            want[v, j] = round(K.eval_error(X[sel], y[sel], Wm, d_in, d_out) * n)
    assert got.tolist() == want.tolist()
    assert len({int(c) for c in got.reshape(-1)}) > 1   # the inputs tell models apart
    # the async form gives the same counts; no inbox gives the base column alone
    assert K.roni_committee_async(X, y, rows, nrows, W, U, cand, d_in, d_out)().tolist() == want.tolist()
    base = K.roni_committee(X, y, rows, nrows, W, U, cand[:, :0], d_in, d_out)
    assert base.tolist() == want[:, :1].tolist()


def _tiny_federation(sizes, d_in, d_out, seed=5):
    rng = np.random.default_rng(seed)
    fed = D.MnistFederation()
    for n in sizes:
        fed.shards_X.append(rng.random((n, d_in), np.float32))
        fed.shards_y.append(rng.integers(0, d_out, n))
    fed.test_X, fed.test_y = rng.random((6, d_in), np.float32), rng.integers(0, d_out, 6)
    fed.attack_X, fed.attack_y = rng.random((3, d_in), np.float32), rng.integers(0, d_out, 3)
    fed.bad_X, fed.bad_y = rng.random((5, d_in), np.float32), rng.integers(0, d_out, 5)
    return fed


def test_softmax_task_roni_rows_match_train_error_minibatches():
    sizes = [23, 31, 4, 17, 12, 40, 10, 9]   # peer 2's and peer 7's shards are shorter than the batch
    task = SoftmaxTask(range(8), 8, "cpu", seed=11, batch_size=10, federation=_tiny_federation(sizes, 70, 3),
                       dims=(70, 3))
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    verifiers, it = [5, 2, 0, 7], 3
    rows, nrows = task.roni_rows(verifiers, it)
    assert rows.shape == (4, 10) and rows.dtype == np.int64 and nrows.dtype == np.int32
    assert nrows.tolist() == [10, 4, 10, 9]
    for k, p in enumerate(verifiers):
        idx = K.minibatch_indices(p, it, sizes[p], 10, 11 ^ 0xB0B)
        n = len(idx)
        assert rows[k, :n].tolist() == [int(offs[p]) + r for r in idx]
        assert (rows[k, n:] == rows[k, n - 1]).all()                       # padded with the last valid row
        assert offs[p] <= rows[k].min() and rows[k].max() < offs[p] + sizes[p]
    # the same rows train_error scores: the committee's base column is train_error(W) per verifier
    W = torch.randn((task.nparam,), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    counts = K.roni_committee(task.X, task.y, torch.from_numpy(rows), torch.from_numpy(nrows), W, None,
                              torch.zeros((4, 0), dtype=torch.int32), 70, 3)
    for k, p in enumerate(verifiers):
        assert counts[k, 0] / nrows[k] == task.train_error(W, p, it)
    # another iteration draws other rows
    assert task.roni_rows(verifiers, it + 1)[0].tolist() != rows.tolist()


def _cpu_engine():
    return BiscottiEngine(RunConfig(num_nodes=8, dataset="mnist", num_verifiers=3, num_miners=1, num_noisers=1,
                                    defense="RONI", device="cpu", seed=7, deterministic_time=True))


def test_cpu_engine_roni_keeps_the_loop(monkeypatch):
    """The batched committee is for the GPU: on the CPU _roni_committee declines and every decision comes from the
    per-candidate train_error loop as before, so the CPU chain is the one it was; it verifies."""
    from biscotti_amd.protocol.verify import VerifyMixin

    declined = []
    orig = VerifyMixin._roni_committee

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        declined.append(out is None)
        return out
    monkeypatch.setattr(VerifyMixin, "_roni_committee", spy)
    eng = _cpu_engine()
    calls = []
    train_error = eng.task.train_error
    eng.task.train_error = lambda *a, **kw: (calls.append(1), train_error(*a, **kw))[1]
    res = [eng.run_round() for _ in range(3)]
    ok, why = eng.fsm.chain.verify()
    assert ok, why
    eng.close()
    assert len(res) == 3 and declined and all(declined)
    # every judged round went through train_error: once for the base model and once per inbox row and verifier
    judged = sum(len(ib) + 1 for r in res for ib in (r.inboxes or {}).values())
    assert len(calls) == judged > 0
