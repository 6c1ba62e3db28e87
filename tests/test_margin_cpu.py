"""The margin-loss local step (the SVM task) without a GPU: the fp64 reference of tests/_margin_ref.py against torch
fp64 autograd, the hinge discontinuity guard on every case, K.margin_step's CPU path against the reference, and the
engines / CLIs with model="svm"."""
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _margin_ref as M
import _ml_ref as R
from biscotti_amd.ops import ml as K

CASES = M.margin_cases()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _step(s, max_norm=100.0):
    d, q, l = K.margin_step(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it,
                            max_norm=max_norm, lo=s.lo)
    return d.numpy().astype(np.float64), q.numpy(), l.numpy().astype(np.float64)


# ---------------------------------------------------------------------------- the reference
def _torch_fp64(s, max_norm=100.0):
    """delta and loss by torch fp64 autograd of F.multi_margin_loss, and the multilabel form's loss."""
    delta, loss, loss_ml = [], [], []
    for p in range(len(s.pid)):
        li = int(s.pid[p]) - s.lo if s.lo >= 0 else p
        idx = K.minibatch_indices(int(s.pid[p]), s.it, int(s.nt[li]), s.B, s.seed)
        rows = [int(s.off[li]) + i for i in idx]
        W = t(s.W).clone().requires_grad_(True)
        xb = (t(s.X)[rows].double() - 0.5) * 2.0
        lab = t(s.y)[rows].long()
        logits = xb @ W[: s.d_out * s.d_in].view(s.d_out, s.d_in).T + W[s.d_out * s.d_in:]
        lv = F.multi_margin_loss(logits, lab, p=1, margin=1.0)
        lv.backward()
        target = torch.full((len(rows), s.d_out), -1, dtype=torch.long)
        target[:, 0] = lab
        loss_ml.append(float(F.multilabel_margin_loss(logits.detach(), target)))
        g = W.grad.numpy()
        coef = max_norm / (np.sqrt((g * g).sum()) + 1e-6)
        delta.append(-(g * coef if coef < 1 else g))
        loss.append(float(lv.detach()))
    return np.stack(delta), np.asarray(loss), np.asarray(loss_ml)


@pytest.mark.parametrize("case", CASES, ids=lambda s: s.name)
def test_reference_matches_torch_fp64_autograd(case):
    d_ref, l_ref, _ = M.margin_refs()[case.name]
    d_t, l_t, l_ml = _torch_fp64(case)
    np.testing.assert_allclose(d_ref, d_t, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(l_ref, l_t, rtol=1e-12, atol=0)
    np.testing.assert_allclose(l_ml, l_t, rtol=1e-12, atol=0)   # the single-target multilabel form: the same loss


def test_case_list_is_the_softmax_list_scaled():
    base = R.softmax_cases()
    assert [c.name for c in CASES] == [c.name for c in base] and len(CASES) == 21
    for a, b in zip(CASES, base):
        assert np.array_equal(a.W, b.W * 4.0) and a.X is b.X and a.y is b.y and a[7:] == b[7:]


@pytest.mark.parametrize("case", CASES, ids=lambda s: s.name)
def test_no_hinge_near_its_kink(case):
    """The discontinuity guard: |z| >= 1e-3 on every hinge of the fp64 reference, so the fp32 paths (logits off by
    a few 1e-6) put every hinge on the reference's side."""
    zs = M.margin_refs()[case.name][2]
    worst = min(float(np.abs(z).min()) for z in zs)
    print(case.name, "min |z|", worst, "active", sum(int((z > 0).sum()) for z in zs), "of", sum(z.size for z in zs))
    assert worst >= M.Z_GUARD


def test_cases_cover_both_branches():
    zs = [z for c in CASES for z in M.margin_refs()[c.name][2]]
    active, total = sum(int((z > 0).sum()) for z in zs), sum(z.size for z in zs)
    assert 0 < active < total
    assert any(bool((z <= 0).all(1).any()) for z in zs), "no fully satisfied row in the case list"
    for c in CASES:   # every case exercises the active branch; the scale keeps a real share of them
        zc = M.margin_refs()[c.name][2]
        assert sum(int((z > 0).sum()) for z in zc) >= 0.5 * sum(z.size for z in zc), c.name


# ---------------------------------------------------------------------------- the CPU path
@pytest.mark.parametrize("case", CASES, ids=lambda s: s.name)
def test_cpu_path_matches_reference(case):
    d_ref, l_ref, _ = M.margin_refs()[case.name]
    d, q, l = _step(case)
    rtol, atol = case.tol
    print(case.name, "max |delta - ref|", np.abs(d - d_ref).max(), "max |loss - ref|", np.abs(l - l_ref).max())
    np.testing.assert_allclose(d, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q, np.trunc(d * R.QSCALE).astype(np.int64))


def test_cpu_genesis_closed_form():
    s = M.genesis_case()
    d_cf, l_cf = M.genesis_closed_form(s)
    d_ref, l_ref, zs = M.margin_step_ref(s.X, s.y, s.off, s.nt, s.pid, s.W, s.d_in, s.d_out, s.B, s.seed, s.it)
    assert all(np.array_equal(z, np.ones_like(z)) for z in zs)
    np.testing.assert_allclose(d_ref, d_cf, rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(l_ref, l_cf, rtol=1e-15)
    d, q, l = _step(s)
    rtol, atol = s.tol
    np.testing.assert_allclose(d, d_cf, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_cf, rtol=1e-6)   # nine exact ones over ten, averaged: a few fp32 roundings
    np.testing.assert_array_equal(q, np.trunc(d * R.QSCALE).astype(np.int64))


@pytest.mark.parametrize("make", [M.tie_case, M.satisfied_case], ids=["tie", "satisfied"])
def test_cpu_tie_and_satisfied_are_all_zero(make):
    s = make()
    d_ref, l_ref, zs = M.margin_step_ref(s.X, s.y, s.off, s.nt, s.pid, s.W, s.d_in, s.d_out, s.B, s.seed, s.it)
    want = 0.0 if make is M.tie_case else -1.0
    assert all(np.array_equal(z, np.full_like(z, want)) for z in zs)
    assert not d_ref.any() and not l_ref.any()
    d, q, l = _step(s)
    assert not d.any() and not q.any() and not l.any()


def test_cpu_clip_case():
    s, (d_ref, l_ref, _) = M.clip_case()
    d_free = M.margin_refs()[s.name][0]
    norms = np.sqrt((d_free * d_free).sum(1))
    assert (norms > M.CLIP_NORM).all()                 # coef < 1 for every peer
    np.testing.assert_allclose(np.sqrt((d_ref * d_ref).sum(1)), M.CLIP_NORM * norms / (norms + 1e-6), rtol=1e-12)
    d, q, l = _step(s, M.CLIP_NORM)
    rtol, atol = s.tol
    np.testing.assert_allclose(d, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q, np.trunc(d * R.QSCALE).astype(np.int64))


def test_softmax_step_cpu_path_is_unchanged_by_the_shared_code():
    """softmax_step and margin_step share one CPU body: the cross-entropy form still matches its fp64 reference."""
    s = R.softmax_cases()[5]
    d_ref, l_ref = R.softmax_refs()[s.name]
    d, q, l = K.softmax_step(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it,
                             lo=s.lo)
    np.testing.assert_allclose(d.numpy(), d_ref, rtol=s.tol[0], atol=s.tol[1])
    np.testing.assert_allclose(l.numpy(), l_ref, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------- engines and CLIs
ROUNDS = 3


def _cfg(**kw):
    from biscotti_amd.protocol.config import RunConfig

    base = dict(num_nodes=12, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True, device="cpu")
    base.update(kw)
    return RunConfig(**base)


def _chain(model):
    from biscotti_amd.protocol.engine import BiscottiEngine

    eng = BiscottiEngine(_cfg(), model=model) if model is not None else BiscottiEngine(_cfg())
    try:
        res = [eng.run_round() for _ in range(ROUNDS)]
        eng.drain()
        ok, why = eng.fsm.chain.verify()
        assert ok, why
        return {"model": eng.model, "loss": eng.task.loss, "empty": [r.empty for r in res],
                "hashes": [bytes(r.block_hash) for r in res],
                "w1": np.array(eng.fsm.chain.block(1).data.global_w),
                "w2": np.array(eng.fsm.chain.block(2).data.global_w)}
    finally:
        eng.close()


@lru_cache(maxsize=None)
def _svm_chain():
    return _chain("svm")


def test_engine_svm_chain_verifies_and_is_reproducible():
    a, b = _svm_chain(), _chain("svm")
    assert a["model"] == "svm" and a["loss"] == "margin" and not a["empty"][0]
    assert a["hashes"] == b["hashes"] and len(set(a["hashes"])) == ROUNDS
    assert np.array_equal(a["w1"], b["w1"]) and np.array_equal(a["w2"], b["w2"])


def test_engine_svm_trains_another_model_than_softmax():
    """The two models part at block 2, not at block 1: at the genesis model W = 0 the two gradients coincide --
    softmax gives (1/C - onehot) / Bq, the margin 1 / (C Bq) off the label and -(C - 1) / (C Bq) on it, the same
    numbers -- so round 0's updates, and with them block 1, agree up to fp32 rounding (not asserted: a rounding
    at a quantisation boundary may show).  From W != 0 on they differ."""
    svm, soft = _svm_chain(), _chain(None)
    assert soft["model"] == "softmax" and soft["loss"] == "ce" and not any(soft["empty"][:2])
    assert not any(svm["empty"][:2]) and svm["w1"].any()
    assert svm["w2"].shape == soft["w2"].shape and not np.array_equal(svm["w2"], soft["w2"])
    assert svm["hashes"][1:] != soft["hashes"][1:]


def test_unknown_model_and_svm_on_creditcard_raise():
    from biscotti_amd.models import make_task
    from biscotti_amd.protocol.engine import BiscottiEngine
    from biscotti_amd.protocol.fedsys import FedSysEngine

    with pytest.raises(ValueError):
        BiscottiEngine(_cfg(), model="perceptron")
    with pytest.raises(ValueError):
        BiscottiEngine(_cfg(dataset="creditcard"), model="svm")
    with pytest.raises(ValueError):
        FedSysEngine(_cfg(dataset="creditcard"), model="svm")
    with pytest.raises(ValueError):
        make_task("mnist", range(2), 2, "cpu", 0, model="cnn")
    with pytest.raises(ValueError):
        make_task("creditcard", range(2), 2, "cpu", 0, model="svm")


def test_fedsys_engine_runs_the_svm():
    from biscotti_amd.protocol.fedsys import FedSysEngine

    eng = FedSysEngine(_cfg(perc_samples=50), model="svm")
    assert eng.model == "svm" and eng.task.loss == "margin"
    res = [eng.run_round() for _ in range(ROUNDS)]
    assert all(r is not None and len(r.selected) > 0 for r in res)
    assert eng.W.abs().sum() > 0 and len(eng.model_digest()) == 64
    assert FedSysEngine(_cfg(perc_samples=50)).model == "softmax"


def test_parsers_take_model_and_default_to_softmax():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.protocol.config import RunConfig, config_from_args

    for mod in (peer, fedsys):
        ap = mod.build_parser()
        assert ap.parse_args(["--model", "svm"]).model == "svm"
        assert ap.parse_args([]).model == "softmax"
        with pytest.raises(SystemExit):
            ap.parse_args(["--model", "cnn"])
    assert config_from_args(peer.build_parser().parse_args(["--model", "svm"])) == RunConfig()


def test_model_is_no_runconfig_field():
    from biscotti_amd.protocol.config import RunConfig

    assert len(fields(RunConfig)) == 51 and "model" not in {f.name for f in fields(RunConfig)}


def test_sandbox_margin_loss_trains_the_svm():
    from biscotti_amd.sandbox import run

    res = run("svm", "creditcard", clients=4, iters=30, eval_every=29, device="cpu", verbose=False, loss="margin")
    assert res["loss"] == "margin" and res["history"][-1]["loss"] < res["history"][0]["loss"]
    assert run("svm", "creditcard", clients=4, iters=2, eval_every=1, device="cpu", verbose=False)["loss"] == "ce"
