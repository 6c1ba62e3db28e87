"""Logistic scoring on the GPU (k_logit_counts): one launch counts the rows that sign(x . w') != y gets wrong, on two
row sets, under the base model and under W + U[c] for every selected candidate.  Its counts equal a float64 numpy
reference exactly on inputs whose every (row, model) is decisive or exactly zero (_logit_ref.py derives the
threshold), survive queued launches, equal the unchanged per-candidate path of LogisticTask, and leave the engine's
chain unchanged while replacing the RONI loop and the blocking evaluation."""
import functools

import numpy as np
import pytest
import torch

import _logit_ref as R
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu

ROWS, MODELS = K.LOGIT_ROWS, K.LOGIT_MODELS

# (N, D, split, nsel): the smallest shapes that reach each path of the kernel
SHAPES = {
    "part_of_one_wave": (9, 25, 4, 1),
    "one_wave": (64, 25, 20, 3),
    "one_wave_and_a_row": (65, 25, 64, 3),
    "block_minus_one": (ROWS - 1, 25, 70, 2),
    "one_block": (ROWS, 25, 70, 2),
    "block_plus_one": (ROWS + 1, 25, ROWS, 2),        # the second block holds one row, all of it set 1
    "split_zero": (200, 25, 0, 2),
    "split_all": (200, 25, 200, 2),
    "split_inside_a_wave": (200, 25, 150, 2),         # rows 128..191 are one wave holding both sets
    "one_feature": (150, 1, 33, 4),
    "d_max": (150, 32, 33, 4),
    "base_only": (150, 25, 33, 0),
    "one_model_tile": (150, 25, 33, MODELS - 1),      # M = the models of one block
    "tile_plus_one": (150, 25, 33, MODELS),           # the base model + a full tile's updates: two tiles
    "tile_plus_two": (150, 25, 33, MODELS + 1),
    "three_tiles_several_blocks": (3 * ROWS + 17, 25, 2 * ROWS + 5, 36),
}


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """Seeded inputs (built once per shape, never modified): X standard normal behind a bias column of ones,
    labels +-1, W standard normal, U = 0.1 N(0, 1) fp32, sel a random draw of candidate rows; the reference's
    counts, which assert that every (row, model) is decisive."""
    N, D, split, nsel = SHAPES[name]
    g = torch.Generator().manual_seed(4000 + seed)
    X = torch.randn((N, D), generator=g, dtype=torch.float64)
    X[:, 0] = 1.0
    y = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).double()
    W = torch.randn((D,), generator=g, dtype=torch.float64)
    n_cand = nsel + 3
    U = (0.1 * torch.randn((n_cand, D), generator=g, dtype=torch.float64)).float()
    sel = torch.randint(0, n_cand, (nsel,), generator=g).to(torch.int32)
    host = dict(X=X, y=y, W=W, U=U, sel=sel)
    want = R.reference(X.numpy(), y.numpy(), split, W.numpy(), U.numpy(), sel.numpy())
    return split, host, {k: t.cuda() for k, t in host.items()}, want


def _counts(dev, split, **over):
    a = dict(dev, **over)
    nsel = a["sel"] is not None and a["sel"].numel()
    return K.logit_counts(a["X"], a["y"], split, a["W"], a["U"] if nsel else None, a["sel"] if nsel else None)


@pytest.mark.parametrize("name", list(SHAPES))
def test_counts_equal_the_fp64_reference(name):
    split, host, dev, want = _case(name)
    N, nsel = host["X"].shape[0], host["sel"].numel()
    got = _counts(dev, split)
    print(name, "margin", R.min_margin(host["X"].numpy(), host["W"].numpy(), host["U"].numpy(), host["sel"].numpy()),
          "got", got.tolist(), "want", want.tolist())
    assert got.shape == (nsel + 1, 2) and got.dtype == np.uint32
    assert got.tolist() == want.tolist()
    assert (got[:, 0] <= split).all() and (got[:, 1] <= N - split).all()


def test_repeated_and_out_of_range_candidates():
    """A repeated sel entry repeats its column; -1 and n_cand score as the base model (and read nothing of U)."""
    split, host, dev, _ = _case("three_tiles_several_blocks")
    n_cand = host["U"].shape[0]
    sel = torch.tensor([5, -1, 7, 5, n_cand, 0, -7, n_cand + 100], dtype=torch.int32)
    want = R.reference(host["X"].numpy(), host["y"].numpy(), split, host["W"].numpy(), host["U"].numpy(), sel.numpy())
    got = _counts(dev, split, sel=sel.cuda())
    assert got.tolist() == want.tolist()
    assert got[1].tolist() == got[4].tolist() != got[0].tolist()
    for m in (2, 5, 7, 8):
        assert got[m].tolist() == got[0].tolist()


def test_zero_margins_count_as_wrong():
    """sign(0) = 0 is wrong like torch.sign: under W = 0 (the genesis model) every count equals its set's size, and
    one all-zero row is wrong under every model."""
    split, host, dev, want = _case("three_tiles_several_blocks")
    N = host["X"].shape[0]
    zero = _counts(dev, split, W=torch.zeros_like(dev["W"]), sel=None)
    assert zero.tolist() == [[split, N - split]]
    X0 = host["X"].clone()
    X0[split + 3] = 0.0
    want0 = R.reference(X0.numpy(), host["y"].numpy(), split, host["W"].numpy(), host["U"].numpy(),
                        host["sel"].numpy())
    was_right = R.reference(host["X"][split + 3:split + 4].numpy(), host["y"][split + 3:split + 4].numpy(), 0,
                            host["W"].numpy(), host["U"].numpy(), host["sel"].numpy())[:, 1] == 0
    assert was_right.any()                                   # the row was right under some model before
    assert (want0[:, 1] - want[:, 1]).tolist() == was_right.astype(int).tolist()
    assert _counts(dev, split, X=X0.cuda()).tolist() == want0.tolist()


def test_out_of_contract_is_an_error_without_a_launch():
    """D = 33 raises.  The launcher itself returns -1 for every out-of-contract argument before it touches the
    stream: the pinned buffer keeps its sentinel.  N == 0 returns 0 and launches nothing either."""
    from biscotti_amd.native import hip

    X = torch.zeros((8, 33), dtype=torch.float64).cuda()
    y = torch.ones((8,), dtype=torch.float64).cuda()
    W = torch.zeros((33,), dtype=torch.float64).cuda()
    with pytest.raises(RuntimeError):
        K.logit_counts(X, y, 0, W)
    dev = torch.zeros((2, 2), dtype=torch.int32).cuda()
    host = torch.full((2, 2), 0x5A5A, dtype=torch.int32).pin_memory()
    U = torch.zeros((1, 33), dtype=torch.float32).cuda()
    sel = torch.zeros((1,), dtype=torch.int32).cuda()

    def launch(N, D, split, M, n_cand):
        return hip().bsc_logit_counts_rb(X.data_ptr(), y.data_ptr(), N, D, split, W.data_ptr(), U.data_ptr(), n_cand,
                                         sel.data_ptr(), M, dev.data_ptr(), host.data_ptr(), K._stream())
    assert launch(8, 33, 0, 1, 0) == -1
    assert launch(8, 0, 0, 1, 0) == -1
    assert launch(-1, 25, 0, 1, 0) == -1
    assert launch(8, 25, 9, 1, 0) == -1
    assert launch(8, 25, -1, 1, 0) == -1
    assert launch(8, 25, 0, 2, 0) == -1
    assert launch(0, 25, 0, 1, 0) == 0
    torch.cuda.synchronize()
    assert host.tolist() == [[0x5A5A] * 2] * 2 and dev.cpu().tolist() == [[0, 0], [0, 0]]
    assert K.logit_counts(X[:0, :25].contiguous(), y[:0], 0, W[:25].contiguous()).tolist() == [[0, 0]]


def test_queued_launches_keep_their_own_results():
    """Two launches queued before either is read, with different updates, on the several-block shape (counters
    accumulated by atomics, so a counter not re-zeroed or a shared read-back buffer would show), then a third."""
    split, host, dev, want1 = _case("three_tiles_several_blocks")
    U2 = (-3.0 * host["U"]).contiguous()
    want2 = R.reference(host["X"].numpy(), host["y"].numpy(), split, host["W"].numpy(), U2.numpy(),
                        host["sel"].numpy())
    assert want1[1:].tolist() != want2[1:].tolist()   # the two launches differ
    a = (dev["X"], dev["y"], split, dev["W"])
    first = K.logit_counts_async(*a, dev["U"], dev["sel"])
    second = K.logit_counts_async(*a, U2.cuda(), dev["sel"])
    assert callable(first.ready) and callable(second.ready)
    got2, got1 = second(), first()
    assert first.ready() and second.ready()
    assert got1.tolist() == want1.tolist() and got2.tolist() == want2.tolist()
    assert K.logit_counts(*a, dev["U"], dev["sel"]).tolist() == want1.tolist()
    assert got1.tolist() == want1.tolist()   # a result already read is not overwritten by the later launches


# ------------------------------------------------------------------ LogisticTask on the real rows
@functools.lru_cache(maxsize=None)
def _task():
    from biscotti_amd.models.tasks import LogisticTask

    return LogisticTask(range(12), 12, torch.device("cuda", 0), 2)


@functools.lru_cache(maxsize=None)
def _real():
    """W = 0.1 N(0, 1) and 36 candidates 0.01 N(0, 1) on the real rows, shown decisive by the reference."""
    t = _task()
    g = torch.Generator().manual_seed(7)
    W = 0.1 * torch.randn((25,), generator=g, dtype=torch.float64)
    U = (0.01 * torch.randn((36, 25), generator=g, dtype=torch.float64)).float()
    X, y = t.eval_X.cpu().numpy(), t.eval_y.cpu().numpy()
    want = R.reference(X, y, t.eval_split, W.numpy(), U.numpy(), np.arange(36))
    want0 = R.reference(X, y, t.eval_split, np.zeros(25), U.numpy(), np.arange(36))   # the genesis model's round
    return W, U, want, want0


def test_committee_equals_train_error_per_candidate():
    """A 3-verifier, 6-slot committee through LogisticTask.roni_committee_async: every column equals
    round(train_error * n_valid) of the unchanged per-candidate path on the GPU, and the reference's count."""
    t = _task()
    W, U, want, _ = _real()
    Wd, Ud = W.cuda(), U.cuda()
    cand = np.asarray([[0, 5, 7, 9, 11, 35], [5, 0, 7, 1, 2, 3], [35, 34, 33, 5, 0, 9]], np.int32)
    counts, nrows = t.roni_committee_async(Wd, Ud, cand)()
    nv = t.Xv.shape[0]
    assert counts.shape == (3, 7) and counts.dtype == np.uint32 and list(nrows) == [nv] * 3
    for v in range(3):
        assert int(counts[v, 0]) == round(t.train_error(Wd, v, 1) * nv) == int(want[0, 1])
        for j, c in enumerate(cand[v]):
            loop = round(t.train_error(Wd + Ud[int(c)].double(), v, 1) * nv)
            print("verifier", v, "slot", j, "committee", int(counts[v, 1 + j]), "loop", loop)
            assert int(counts[v, 1 + j]) == loop == int(want[1 + int(c), 1])


@pytest.mark.parametrize("zero", [True, False], ids=["genesis_model", "random_model"])
def test_evaluation_equals_err_on_both_sets(zero):
    t = _task()
    W, _, want, _ = _real()
    Wd = torch.zeros_like(W).cuda() if zero else W.cuda()
    ev = t.evaluate(Wd)
    nt, nv = t.Xt.shape[0], t.Xv.shape[0]
    print(ev, t._err(t.Xt, t.yt, Wd), t._err(t.Xv, t.yv, Wd))
    assert ev == {"test_error": t._err(t.Xt, t.yt, Wd), "valid_error": t._err(t.Xv, t.yv, Wd), "attack_rate": 0.0}
    if zero:
        assert ev["test_error"] == 1.0 and ev["valid_error"] == 1.0
    else:
        assert ev["test_error"] == int(want[0, 0]) / nt and ev["valid_error"] == int(want[0, 1]) / nv


def test_queued_evaluations_read_in_reverse_order():
    t = _task()
    W, U, want, want0 = _real()
    nt, nv = t.Xt.shape[0], t.Xv.shape[0]
    W2 = W + U[4].double()
    first, second = t.evaluate_async(W.cuda()), t.evaluate_async(W2.cuda())
    assert callable(first.ready) and callable(second.ready)
    e2, e1 = second(), first()
    assert first.ready() and second.ready()
    assert (e1["test_error"], e1["valid_error"]) == (int(want[0, 0]) / nt, int(want[0, 1]) / nv)
    assert (e2["test_error"], e2["valid_error"]) == (int(want[5, 0]) / nt, int(want[5, 1]) / nv)
    assert e1["attack_rate"] == 0.0 and want[0].tolist() != want[5].tolist()


# ------------------------------------------------------------------ the engine
def _engine(**kw):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    base = dict(num_nodes=12, dataset="creditcard", seed=2, defense="RONI", deterministic_time=True)
    base.update(kw)
    return BiscottiEngine(RunConfig(**base), Comm(device=torch.device("cuda", 0)))


def test_accept_matrix_equals_the_verify_loop():
    """_roni_committee against _verify on one engine, same model and candidates: the same accept matrix."""
    W, U, _, _ = _real()
    t = _task()
    R.reference(t.Xv.cpu().numpy(), t.yv.cpu().numpy(), 0, W.numpy(), (3.0 * U).numpy(), np.arange(36))   # decisive
    eng = _engine()
    try:
        eng.W = W.cuda()
        X = (3.0 * U).cuda().contiguous()   # large enough updates that RONI rejects some
        local_vs = [eng.lo, eng.lo + 1, eng.lo + 2]
        inboxes = {local_vs[0]: [0, 5, 7, 9, 11, 35], local_vs[1]: [5, 0, 7, 1, 2, 3],
                   local_vs[2]: [35, 34, 33, 5, 0, 9]}
        xrow = {w: w for w in range(36)}
        got = eng._roni_committee(X, xrow, inboxes, local_vs, 1)
        want = [eng._verify(X[inboxes[v]].contiguous(), inboxes[v], 1, v) for v in local_vs]
    finally:
        eng.close()
    print("accepts", np.asarray(got).astype(int).tolist())
    assert got is not None and np.asarray(got).tolist() == want
    assert 0 < int(np.asarray(got).sum()) < 18   # both decisions occur


def _run(monkeypatch, rounds, batched, **kw):
    """`rounds` RONI rounds; batched False forces the per-candidate loop.  Returns the results, the models of each
    committee launch and the number of train_error calls."""
    from biscotti_amd.protocol.verify import VerifyMixin

    launches, train_calls = [], []
    with monkeypatch.context() as m:
        if not batched:
            m.setattr(VerifyMixin, "_roni_committee", lambda self, *a, **k: None)
        real = K.logit_counts_async

        def spy(X, y, split, W, U=None, sel=None):
            if sel is not None:   # a committee (the evaluation passes no candidates)
                launches.append(1 + sel.numel())
            return real(X, y, split, W, U, sel)
        m.setattr(K, "logit_counts_async", spy)
        eng = _engine(**kw)
        train_error = eng.task.train_error
        eng.task.train_error = lambda *a, **k: (train_calls.append(1), train_error(*a, **k))[1]
        res = [eng.run_round() for _ in range(rounds)]
        ok, why = eng.fsm.chain.verify()
        eng.close()
    assert ok, why
    return res, launches, len(train_calls)


@pytest.mark.parametrize("kw", [{}, {"poisoning": 0.3}], ids=["honest", "poisoning_0.3"])
def test_engine_chain_equals_the_loop(monkeypatch, kw):
    res, launches, train_calls = _run(monkeypatch, 3, batched=True, **kw)
    ref, ref_launches, ref_train_calls = _run(monkeypatch, 3, batched=False, **kw)
    assert [bytes(r.block_hash) for r in res] == [bytes(r.block_hash) for r in ref]
    for r, q in zip(res, ref):
        assert r.approved == q.approved and r.node_list == q.node_list
        assert r.test_error == q.test_error
    assert sum(not r.empty for r in res) >= 2
    judged = [r for r in res if r.inboxes]
    assert len(launches) == len(judged) >= 2 and all(n >= 2 for n in launches)   # once per judged round
    assert train_calls == 0
    assert ref_launches == [] and ref_train_calls > 0                            # the forced run took the loop
