"""Committee RONI on the GPU (k_roni_counts): one launch scores every verifier's minibatch under the base model and
under every update of its inbox.  Its counts equal the per-candidate k_eval_error loop's exactly, agree with an fp64
host evaluation wherever that one is decisive, survive queued launches, and leave the engine's chain unchanged."""
import functools

import numpy as np
import pytest
import torch

from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu

# (d_in, d_out, V, ni, B, nrows): the smallest shapes that reach each path of the kernel
SHAPES = {
    "mnist_main_loop_and_tail": (784, 10, 3, 7, 10, None),     # 196 K per wave: six 32-wide steps + one 4-wide
    "tail_only_guard": (70, 3, 2, 5, 10, None),                # 20 K per wave, the last wave 10: k < kend, D_OUT < 16
    "lfw_dims": (8742, 2, 2, 3, 10, None),                     # D_IN % 4 == 2, two classes
    "two_tiles": (784, 10, 2, 4, 17, None),                    # second tile holds one row: the atomic path
    "full_tile": (784, 10, 2, 4, 16, None),
    "short_minibatch": (784, 10, 3, 4, 10, (10, 3, 10)),       # nrows < Bmax: clamped loads, never counted
    "one_by_one": (784, 10, 1, 1, 10, None),
}
FP64_SHAPES = ("mnist_main_loop_and_tail", "tail_only_guard", "lfw_dims", "two_tiles")


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """Seeded inputs on the device (built once per shape, never modified): X uniform [0, 1), random labels,
    W standard normal, U = 0.1 N(0, 1) fp32."""
    d_in, d_out, V, ni, B, nr = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    n_rows, n_cand = (64 if d_in > 1000 else 200), ni + 3
    X = torch.rand((n_rows, d_in), generator=g, dtype=torch.float32)
    y = torch.randint(0, d_out, (n_rows,), generator=g, dtype=torch.int32)
    W = torch.randn((d_out * d_in + d_out,), generator=g, dtype=torch.float64)
    U = 0.1 * torch.randn((n_cand, d_out * d_in + d_out), generator=g, dtype=torch.float32)
    nrows = torch.tensor(nr if nr is not None else [B] * V, dtype=torch.int32)
    rows = torch.stack([torch.randperm(n_rows, generator=g)[:B] for _ in range(V)]).to(torch.int64)
    for v in range(V):   # as SoftmaxTask.roni_rows pads: the last valid row repeated
        rows[v, int(nrows[v]):] = rows[v, int(nrows[v]) - 1]
    cand = torch.stack([torch.randperm(n_cand, generator=g)[:ni] for _ in range(V)]).to(torch.int32)
    host = dict(X=X, y=y, W=W, U=U, rows=rows, nrows=nrows, cand=cand)
    dev = {k: t.cuda() for k, t in host.items()}
    return (d_in, d_out, V, ni, B), host, dev


def _committee(dev, d_in, d_out, **over):
    a = dict(dev, **over)
    return K.roni_committee(a["X"], a["y"], a["rows"], a["nrows"], a["W"], a["U"], a["cand"], d_in, d_out)


def _loop_counts(host, dev, d_in, d_out):
    """The unchanged path: one k_eval_error launch per (verifier, model) on the gathered rows, as
    SoftmaxTask.train_error runs it."""
    V, ni = host["cand"].shape
    out = np.zeros((V, ni + 1), np.int64)
    for v in range(V):
        n = int(host["nrows"][v])
        sel = dev["rows"][v, :n]
        Xv, yv = dev["X"][sel].contiguous(), dev["y"][sel].contiguous()
        models = [dev["W"]] + [dev["W"] + dev["U"][int(c)].double() for c in host["cand"][v]]
        for j, Wm in enumerate(models):
            out[v, j] = round(K.eval_error(Xv, yv, Wm, d_in, d_out, True) * n)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_counts_equal_the_eval_error_loop(name):
    (d_in, d_out, V, ni, B), host, dev = _case(name)
    got = _committee(dev, d_in, d_out)
    assert got.shape == (V, ni + 1) and got.dtype == np.uint32
    want = _loop_counts(host, dev, d_in, d_out)
    print(name, "committee", got.tolist(), "loop", want.tolist())
    assert got.tolist() == want.tolist()
    assert (got <= host["nrows"].numpy()[:, None]).all()


def test_empty_inbox_gives_the_base_column():
    """ni == 0: the result is [V, 1], the base model's counts (one launch of one column); no verifier or no
    minibatch slot gives zeros without a launch."""
    (d_in, d_out, V, ni, B), host, dev = _case("mnist_main_loop_and_tail")
    full = _committee(dev, d_in, d_out)
    base = _committee(dev, d_in, d_out, cand=dev["cand"][:, :0].contiguous())
    assert base.shape == (V, 1) and base.tolist() == full[:, :1].tolist()
    none = _committee(dev, d_in, d_out, rows=dev["rows"][:0].contiguous(), nrows=dev["nrows"][:0].contiguous(),
                      cand=dev["cand"][:0].contiguous())
    assert none.shape == (0, ni + 1)
    assert _committee(dev, d_in, d_out, rows=dev["rows"][:, :0].contiguous()).tolist() == [[0] * (ni + 1)] * V


def test_more_than_sixteen_classes_is_an_error():
    g = torch.Generator().manual_seed(3)
    X = torch.rand((16, 8), generator=g).cuda()
    y = torch.zeros((16,), dtype=torch.int32).cuda()
    W = torch.randn((17 * 8 + 17,), generator=g, dtype=torch.float64).cuda()
    U = torch.zeros((1, 17 * 8 + 17), dtype=torch.float32).cuda()
    rows = torch.arange(10, dtype=torch.int64).view(1, 10).cuda()
    with pytest.raises(RuntimeError):
        K.roni_committee(X, y, rows, torch.tensor([10], dtype=torch.int32).cuda(), W, U,
                         torch.zeros((1, 1), dtype=torch.int32).cuda(), 8, 17)


@pytest.mark.parametrize("name", FP64_SHAPES)
def test_counts_agree_with_fp64_where_it_is_decisive(name):
    """Predictions in float64 on the host; rows whose fp64 top-two logit gap is below 1e-3 * max|logit| are left
    out (fp32 may order them either way).  At most 2.5 % of the (verifier, column, row) triples may be left out
    (the fp64 reference alone stays at or below 1.25 % for these input distributions); over the rest the counts
    match exactly.  A cell with rows left out is scored again by the kernel on its kept rows alone."""
    (d_in, d_out, V, ni, B), host, dev = _case(name)
    got = _committee(dev, d_in, d_out)
    X, y, W, U = host["X"].double(), host["y"].long(), host["W"], host["U"].double()
    triples = excluded = 0
    for v in range(V):
        n = int(host["nrows"][v])
        sel = host["rows"][v, :n]
        xb = (X[sel] - 0.5) * 2.0
        for col in range(ni + 1):
            c = int(host["cand"][v, col - 1]) if col else -1
            Wm = W + U[c] if col else W
            logits = xb @ Wm[: d_out * d_in].view(d_out, d_in).T + Wm[d_out * d_in:]
            top = torch.topk(logits, 2, dim=1).values
            keep = (top[:, 0] - top[:, 1]) >= 1e-3 * logits.abs().max(dim=1).values
            wrong = logits.argmax(1) != y[sel]
            triples += n
            excluded += int((~keep).sum())
            want = int((wrong & keep).sum())
            if bool(keep.all()):
                cell = int(got[v, col])
            elif not bool(keep.any()):
                continue
            else:   # the kernel on the kept rows of this (verifier, model) alone
                kept = sel[keep].view(1, -1).cuda().contiguous()
                cd = torch.tensor([[max(c, 0)]], dtype=torch.int32).cuda()
                one = _committee(dev, d_in, d_out, rows=kept, cand=cd,
                                 nrows=torch.tensor([kept.shape[1]], dtype=torch.int32).cuda())
                cell = int(one[0, 1 if col else 0])
            assert cell == want, (name, v, col, cell, want)
    print(name, "excluded", excluded, "of", triples)
    assert excluded <= 0.025 * triples, (excluded, triples)


def test_queued_committees_keep_their_own_results():
    """Two committees queued before either is read, with different updates, on the several-tile shape (counters
    accumulated by atomics, so a counter not re-zeroed or a shared read-back buffer would show), then a third."""
    (d_in, d_out, V, ni, B), host, dev = _case("two_tiles")
    U2 = (-3.0 * dev["U"]).contiguous()
    a = (dev["X"], dev["y"], dev["rows"], dev["nrows"], dev["W"])
    first = K.roni_committee_async(*a, dev["U"], dev["cand"], d_in, d_out)
    second = K.roni_committee_async(*a, U2, dev["cand"], d_in, d_out)
    got2, got1 = second(), first()
    want1 = _loop_counts(host, dev, d_in, d_out)
    want2 = _loop_counts(dict(host, U=-3.0 * host["U"]), dict(dev, U=U2), d_in, d_out)
    assert want1[:, 1:].tolist() != want2[:, 1:].tolist()   # the two committees differ
    assert got1.tolist() == want1.tolist() and got2.tolist() == want2.tolist()
    assert K.roni_committee(*a, dev["U"], dev["cand"], d_in, d_out).tolist() == want1.tolist()
    assert got1.tolist() == want1.tolist()   # a result already read is not overwritten by the later launches


def _engine(**kw):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    base = dict(num_nodes=12, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True, defense="RONI")
    base.update(kw)
    return BiscottiEngine(RunConfig(**base), Comm(device=torch.device("cuda", 0)))


def _run(monkeypatch, rounds, batched, **kw):
    """`rounds` RONI rounds; batched False forces the per-candidate loop.  Returns the results, the number of
    committee launches and of train_error calls."""
    from biscotti_amd.protocol.verify import VerifyMixin

    launches, train_calls = [], []
    with monkeypatch.context() as m:
        if not batched:
            m.setattr(VerifyMixin, "_roni_committee", lambda self, *a, **k: None)
        real = K.roni_committee_async

        def spy(X, y, rows, *a, **k):
            launches.append(rows.shape[0])   # the local verifiers judged by this launch
            return real(X, y, rows, *a, **k)
        m.setattr(K, "roni_committee_async", spy)
        eng = _engine(**kw)
        train_error = eng.task.train_error
        eng.task.train_error = lambda *a, **k: (train_calls.append(1), train_error(*a, **k))[1]
        res = [eng.run_round() for _ in range(rounds)]
        ok, why = eng.fsm.chain.verify()
        eng.close()
    assert ok, why
    return res, launches, len(train_calls)


def test_engine_chain_equals_the_loop(monkeypatch):
    res, launches, train_calls = _run(monkeypatch, 3, batched=True)
    ref, ref_launches, ref_train_calls = _run(monkeypatch, 3, batched=False)
    assert [bytes(r.block_hash) for r in res] == [bytes(r.block_hash) for r in ref]
    for r, q in zip(res, ref):
        assert r.approved == q.approved and r.node_list == q.node_list
    assert sum(not r.empty for r in res) >= 2
    judged = [r for r in res if r.inboxes]
    assert len(launches) == len(judged) >= 2 and all(n >= 1 for n in launches)   # once per round, local verifiers
    assert train_calls == 0
    assert ref_launches == [] and ref_train_calls > 0                            # the forced run took the loop


def test_lfw_engine_on_the_committee_path(monkeypatch):
    res, launches, train_calls = _run(monkeypatch, 2, batched=True, dataset="lfw")
    assert len(launches) >= 1 and train_calls == 0
