"""Local multi-step updates without a GPU: K.local_steps' torch fp32 path against the fp64 reference of
tests/_local_ref.py on the cases the kernel is taken to, E = 1 against the single step bit for bit, and the arguments."""
import numpy as np
import pytest
import torch

import _local_ref as L
from biscotti_amd.ops import ml as K

t = torch.from_numpy


def _args(s):
    return t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_cpu_local_steps_match_fp64_reference(case):
    i, loss, E, lr = case
    s, max_norm, _ = L.shapes()[i]
    d_ref, l_ref = L.ref(*case)
    d, q, l = K.local_steps(*_args(s), E, lr, loss=loss, max_norm=max_norm, lo=s.lo)
    rtol, atol = L.tol(s, E)
    np.testing.assert_allclose(d.numpy().astype(np.float64), d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l.numpy().astype(np.float64), l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.numpy(), np.trunc(d.numpy().astype(np.float64) * 1e4).astype(np.int64))


@pytest.mark.parametrize("loss,single", [("ce", K.softmax_step), ("margin", K.margin_step)])
def test_one_local_step_at_rate_one_is_the_single_step(loss, single):
    for s, max_norm, _ in L.shapes()[1:5]:
        one = K.local_steps(*_args(s), 1, 1.0, loss=loss, max_norm=max_norm, lo=s.lo)
        assert all(torch.equal(a, b) for a, b in zip(one, single(*_args(s), max_norm=max_norm, lo=s.lo)))


def test_local_steps_validation_and_parsers():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.models import make_task

    for kw in ({"local_steps": 0}, {"local_steps": 65}, {"local_steps": 2.5}, {"local_lr": 0.0}, {"local_lr": -1.0}):
        with pytest.raises(ValueError, match="local_"):
            make_task("mnist", range(2), 2, "cpu", 0, **kw)
    with pytest.raises(ValueError, match="creditcard"):
        make_task("creditcard", range(2), 2, "cpu", 0, local_steps=2)
    s = L.shapes()[0][0]
    for E, lr in ((0, 1.0), (65, 1.0), (2, 0.0)):
        with pytest.raises(ValueError):
            K.local_steps(*_args(s), E, lr)
    for mod in (peer, fedsys):
        ns = mod.build_parser().parse_args(["--local-steps", "4", "--local-lr", "0.5"])
        assert (ns.local_steps, ns.local_lr) == (4, 0.5)
        ns = mod.build_parser().parse_args([])
        assert (ns.local_steps, ns.local_lr) == (1, 1.0)
