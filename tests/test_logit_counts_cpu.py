"""Logistic miss counts on the CPU (ops.ml.logit_counts, the numpy path beside k_logit_counts): equal to the
LogisticTask._err-based counts on the real creditcard rows, to the float64 reference at the edges, and unused by the
CPU engine's RONI (which keeps the per-candidate loop)."""
import functools

import numpy as np
import pytest
import torch

import _logit_ref as R
from biscotti_amd.ops import ml as K


@functools.lru_cache(maxsize=None)
def _task():
    from biscotti_amd.models.tasks import LogisticTask

    return LogisticTask(range(4), 4, "cpu", 1)


@functools.lru_cache(maxsize=None)
def _inputs():
    """W = 0.1 N(0, 1), 36 candidates 0.01 N(0, 1) fp32 (seeded; never modified)."""
    g = torch.Generator().manual_seed(7)
    W = 0.1 * torch.randn((25,), generator=g, dtype=torch.float64)
    U = (0.01 * torch.randn((36, 25), generator=g, dtype=torch.float64)).float()
    return W, U


def test_resident_evaluation_rows():
    t = _task()
    assert t.eval_X.shape == (t.Xt.shape[0] + t.Xv.shape[0], 25) and t.eval_split == t.Xt.shape[0]
    assert torch.equal(t.eval_X[: t.eval_split], t.Xt) and torch.equal(t.eval_X[t.eval_split:], t.Xv)
    assert torch.equal(t.eval_y[: t.eval_split], t.yt) and torch.equal(t.eval_y[t.eval_split:], t.yv)
    assert t.eval_X.is_contiguous() and t.eval_y.is_contiguous() and t.Xv.shape[0] == 8999


def test_counts_equal_the_err_based_counts_on_the_real_rows():
    """Both sets of the evaluation and every candidate of a committee against LogisticTask._err, after the
    reference has shown every (row, model) decisive (so the matmul's summation order cannot matter)."""
    t = _task()
    W, U = _inputs()
    sel = torch.arange(36, dtype=torch.int32)
    want = R.reference(t.eval_X.numpy(), t.eval_y.numpy(), t.eval_split, W.numpy(), U.numpy(), sel.numpy())
    print("min relative margin", R.min_margin(t.eval_X.numpy(), W.numpy(), U.numpy(), sel.numpy()))
    got = K.logit_counts(t.eval_X, t.eval_y, t.eval_split, W, U, sel)
    assert got.dtype == np.uint32 and got.shape == (37, 2)
    assert got.tolist() == want.tolist()
    nt, nv = t.Xt.shape[0], t.Xv.shape[0]
    for m in range(37):
        Wm = W if m == 0 else W + U[m - 1].double()
        assert int(got[m, 0]) == round(t._err(t.Xt, t.yt, Wm) * nt)
        assert int(got[m, 1]) == round(t._err(t.Xv, t.yv, Wm) * nv)
    ev = t.evaluate(W)
    assert ev == {"test_error": got[0, 0] / nt, "valid_error": got[0, 1] / nv, "attack_rate": 0.0}


def test_zero_model_and_bad_sel():
    """W = 0 (the genesis model): sign(0) = 0 is wrong on every row, so the error is exactly 1.0; a sel entry of -1
    or n_cand scores as the base model; a repeated entry repeats its column."""
    t = _task()
    W, U = _inputs()
    nt, nv = t.Xt.shape[0], t.Xv.shape[0]
    assert K.logit_counts(t.eval_X, t.eval_y, t.eval_split, torch.zeros_like(W)).tolist() == [[nt, nv]]
    assert t.evaluate(torch.zeros_like(W))["test_error"] == 1.0
    sel = torch.tensor([3, -1, 36, 3], dtype=torch.int32)
    got = K.logit_counts(t.Xv, t.yv, 0, W, U, sel)
    assert got.tolist() == R.reference(t.Xv.numpy(), t.yv.numpy(), 0, W.numpy(), U.numpy(), sel.numpy()).tolist()
    assert got[2].tolist() == got[0].tolist() == got[3].tolist() and got[1].tolist() == got[4].tolist()
    assert (got[:, 0] == 0).all()   # split == 0: set 0 is empty


def test_out_of_contract_raises():
    t = _task()
    W, U = _inputs()
    X33 = torch.zeros((4, 33), dtype=torch.float64)
    with pytest.raises(RuntimeError):
        K.logit_counts(X33, torch.ones(4, dtype=torch.float64), 0, torch.zeros(33, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        K.logit_counts(t.Xv, t.yv, t.Xv.shape[0] + 1, W)
    with pytest.raises(RuntimeError):
        K.logit_counts(t.Xv, t.yv, -1, W)
    with pytest.raises(RuntimeError):
        K.logit_counts(t.Xv, t.yv, 0, W, None, torch.zeros(1, dtype=torch.int32))
    assert K.logit_counts(t.Xv[:0], t.yv[:0], 0, W).tolist() == [[0, 0]]


def test_committee_entry_point_broadcasts_per_candidate_counts():
    """LogisticTask.roni_committee_async: counts [V, ni + 1] in roni_accept's form, equal to train_error's count
    per (verifier, model); the accept matrix equals the loop's decisions."""
    t = _task()
    W, U = _inputs()
    cand = np.asarray([[0, 5, 7, 9, 11, 35], [5, 0, 7, 1, 2, 3], [35, 34, 33, 5, 0, 9]], np.int32)
    counts, nrows = t.roni_committee_async(W, U, cand)()
    nv = t.Xv.shape[0]
    assert counts.shape == (3, 7) and list(nrows) == [nv] * 3
    for v in range(3):
        base = t.train_error(W, v, 0)
        assert int(counts[v, 0]) == round(base * nv)
        for j, c in enumerate(cand[v]):
            e = t.train_error(W + U[int(c)].double(), v, 0)
            assert int(counts[v, 1 + j]) == round(e * nv)
            assert bool(K.roni_accept(counts, nrows)[v, j]) == (e - base <= 0.02)


def test_cpu_engine_keeps_the_loop(monkeypatch):
    """_roni_committee returns None on the CPU engine: the per-candidate loop judges, train_error is called."""
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine
    from biscotti_amd.protocol.verify import VerifyMixin

    returned, calls = [], []
    real = VerifyMixin._roni_committee

    def spy(self, *a, **k):
        returned.append(real(self, *a, **k))
        return returned[-1]
    monkeypatch.setattr(VerifyMixin, "_roni_committee", spy)
    launches = []
    real_counts = K.logit_counts_async
    monkeypatch.setattr(K, "logit_counts_async", lambda *a, **k: (launches.append(1), real_counts(*a, **k))[1])
    eng = BiscottiEngine(RunConfig(num_nodes=12, dataset="creditcard", seed=2, defense="RONI", device="cpu",
                                   deterministic_time=True))
    train_error = eng.task.train_error
    eng.task.train_error = lambda *a, **k: (calls.append(1), train_error(*a, **k))[1]
    res = [eng.run_round() for _ in range(2)]
    ok, why = eng.fsm.chain.verify()
    eng.close()
    assert ok, why
    assert returned and all(r is None for r in returned)
    assert calls and not launches
    assert any(not r.empty for r in res)
