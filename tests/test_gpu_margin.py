"""k_margin_step (the SVM task's local step) on the GPU against the fp64 reference of tests/_margin_ref.py (every case
vetted on the CPU by tests/test_margin_cpu.py), its launcher's limits, and the engine with model="svm".

What each group would catch:
  numerics   a hinge counted at z == 0 or at the label's own column; the loss divided by C - 1 or by B instead of
             Bq; the label's gradient without the active count; the K-tile and resident-index mistakes of the
             softmax step, whose body this kernel shares
  launcher   limits or the `ones` flags dropped from the second launcher
  engine     a native pre-step that forgot the loss (it would queue k_softmax_step while the Python step runs
             k_margin_step: the pipelined chain would differ from the unpipelined one)
"""
import numpy as np
import pytest
import torch

import _margin_ref as M
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


def _step(s, max_norm=100.0):
    d, q, l = K.margin_step(c(s.X), c(s.y), c(s.off), c(s.nt), c(s.pid), c(s.W), s.d_in, s.d_out, s.B, s.seed, s.it,
                            max_norm=max_norm, lo=s.lo)
    return f64(d), q.cpu().numpy(), f64(l)


def _check(s, d_ref, l_ref, max_norm=100.0):
    d, q, l = _step(s, max_norm)
    rtol, atol = s.tol
    print(s.name, "max |delta - ref|", np.abs(d - d_ref).max(), "max |loss - ref|", np.abs(l - l_ref).max())
    np.testing.assert_allclose(d, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    # exact: Go's int64(float64(delta) * 10^precision) of the kernel's own delta
    np.testing.assert_array_equal(q, np.trunc(d * R.QSCALE).astype(np.int64))


# ---------------------------------------------------------------------------- kernel numerics
@pytest.mark.parametrize("case", M.margin_cases(), ids=lambda s: s.name)
def test_margin_step_edges(case):
    d_ref, l_ref, zs = M.margin_refs()[case.name]
    assert min(float(np.abs(z).min()) for z in zs) >= M.Z_GUARD   # no hinge can change side in fp32
    _check(case, d_ref, l_ref)


def test_margin_genesis_closed_form():
    s = M.genesis_case()
    d_cf, l_cf = M.genesis_closed_form(s)
    _check(s, d_cf, np.full(len(s.pid), l_cf))
    l = _step(s)[2]
    np.testing.assert_allclose(l, l_cf, rtol=1e-6)   # nine exact ones over ten, averaged: a few fp32 roundings


@pytest.mark.parametrize("make", [M.tie_case, M.satisfied_case], ids=["tie", "satisfied"])
def test_margin_tie_and_satisfied_are_all_zero(make):
    """z == 0 exactly (tie) or z == -1 (satisfied) on every hinge: nothing is active, every output bit is zero
    (a negative zero in delta is a zero)."""
    d, q, l = _step(make())
    assert not d.any() and not q.any() and not l.any()


def test_margin_clip():
    s, (d_ref, l_ref, _) = M.clip_case()
    _check(s, d_ref, l_ref, M.CLIP_NORM)
    d = _step(s, M.CLIP_NORM)[0]
    np.testing.assert_allclose(np.sqrt((d * d).sum(1)), M.CLIP_NORM, rtol=1e-4)


def test_margin_differs_from_softmax_step():
    s = M.margin_cases()[5]
    d_sm = K.softmax_step(c(s.X), c(s.y), c(s.off), c(s.nt), c(s.pid), c(s.W), s.d_in, s.d_out, s.B, s.seed, s.it,
                          lo=s.lo)[0]
    assert np.abs(f64(d_sm) - _step(s)[0]).max() > 1e-3


# ---------------------------------------------------------------------------- launcher
def _margin_raw(d_in, d_out, B, ones=None, nones=0):
    n = 4
    X, y = torch.rand((n, max(d_in, 1))).cuda(), torch.zeros(n, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), i32([n]), i32([0])
    nparam = d_out * d_in + d_out
    W = torch.zeros(max(nparam, 1), dtype=torch.float64).cuda()
    delta = torch.zeros((1, max(nparam, 1)), dtype=torch.float32).cuda()
    qdelta = torch.zeros((1, max(nparam, 1)), dtype=torch.int64).cuda()
    loss = torch.zeros(1, dtype=torch.float32).cuda()
    rc = hip().bsc_margin_step(X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(), W.data_ptr(),
                               d_in, d_out, B, 1, 7, 0, 100.0, R.QSCALE, delta.data_ptr(), qdelta.data_ptr(),
                               loss.data_ptr(), -1, None if ones is None else ones.data_ptr(), nones,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_margin_launcher_limits_and_ones():
    assert _margin_raw(8, 17, 4) == -1
    assert _margin_raw(8, 4, 17) == -1
    assert _margin_raw(0, 4, 4) == -1
    ones = torch.full((301,), -7, dtype=torch.int32).cuda()
    assert _margin_raw(8, 4, 4, ones, 300) == 0
    assert ones.cpu().tolist() == [1] * 300 + [-7]      # more than one pass of the 256 threads; the canary stays


# ---------------------------------------------------------------------------- engine
def _engine(model="svm", **kw):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    base = dict(num_nodes=12, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True)
    base.update(kw)
    return BiscottiEngine(RunConfig(**base), Comm(device=torch.device("cuda", 0)), model=model)


def _run_exact(eng, rounds=4):
    seen = {}
    step = eng.task.step

    def spy(W, it, peers):  # record every peer's quantised update as the engine computes it
        d, q = step(W, it, peers)
        seen.update({(it, p): q[i].clone() for i, p in enumerate(peers)})
        return d, q
    eng.task.step = spy
    if eng._native is not None:
        # the pre-step runs natively (NativeSecAgg.prestep / after_select): record its quantised updates too
        pre_fn = eng._native._pre_out

        def pre_spy(k, W, it):
            out = pre_fn(k, W, it)
            torch.cuda.current_stream().wait_event(out["ev"])   # the step runs on the Gram stream
            seen.update({(it, p): out["qdelta"][i].clone() for i, p in enumerate(eng.task.peers)})
            return out
        eng._native._pre_out = pre_spy
    res = []
    for _ in range(rounds):
        W0 = eng.W.clone()
        r = eng.run_round()
        res.append(r)
        if not r.empty and eng.cfg.secure_agg:
            q = torch.stack([seen[(r.iteration, p)] for p in r.node_list])
            torch.testing.assert_close(eng.W, W0 + q.sum(0).double() / 10.0 ** eng.cfg.precision, rtol=0,
                                       atol=1e-12)
    ok, why = eng.fsm.chain.verify()
    assert ok, why
    native_step = eng._native is not None and eng._native.task is not None
    eng.close()
    return res, native_step


@pytest.mark.parametrize("defense", ["KRUM", "RONI"])
def test_svm_engine_exact_and_pipelined_chain_equals_unpipelined(defense):
    """The exact-aggregation invariant with model="svm", and the chain of the pipelined run (the pre-step queued
    natively, bsc_round_prestep_slot) byte for byte the chain of the unpipelined one (the Python step)."""
    out = []
    for abl in ("", "no_pipeline"):
        eng = _engine(defense=defense, ablation=abl)
        assert eng.model == "svm" and eng.task.loss == "margin"
        res, native_step = _run_exact(eng)
        assert any(not r.empty for r in res)
        out.append(([bytes(r.block_hash) for r in res], native_step))
    (h_pipe, native_pipe), (h_plain, native_plain) = out
    assert native_pipe and not native_plain     # the two runs did take the two step paths
    assert h_pipe == h_plain and len(set(h_pipe)) == 4


def test_svm_learns():
    """20 peers, 30 rounds: the final test error is below the genesis model's on the same test rows."""
    eng = _engine(num_nodes=20)
    genesis = eng.task.evaluate(eng.W)["test_error"]
    res = [eng.run_round() for _ in range(30)]
    eng.drain()
    ok, why = eng.fsm.chain.verify()
    final = eng.task.evaluate(eng.W)["test_error"]
    eng.close()
    assert ok, why
    print("svm test error: genesis", genesis, "after 30 rounds", final, "non-empty blocks",
          sum(not r.empty for r in res))
    assert final < genesis
