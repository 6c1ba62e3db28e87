"""DP-SGD local steps without a GPU: K.dpsgd_steps' torch fp32 path against the fp64 reference of tests/_dpsgd_ref.py on
the cases the kernel is taken to, and the arguments."""
import os
import sys

import numpy as np
import pytest
import torch

import _dpsgd_ref as DP
from biscotti_amd.ops import ml as K

t = torch.from_numpy


def _args(s):
    return t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it


@pytest.mark.parametrize("case", DP.CASES, ids=DP.case_id)
def test_cpu_dpsgd_steps_match_fp64_reference(case):
    i, loss, E, lr, _, S = case
    s = DP.shapes()[i]
    d_ref, l_ref, bq, C = DP.ref(*case)
    d, q, l = K.dpsgd_steps(*_args(s), C, S, E, lr, loss=loss, lo=s.lo)
    d = d.numpy().astype(np.float64)
    rtol, atol = DP.tol(s, E, lr, S, C, bq)
    assert (np.abs(d - d_ref) <= atol + rtol * np.abs(d_ref)).all()
    np.testing.assert_allclose(l.numpy().astype(np.float64), l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.numpy(), np.trunc(d * 1e4).astype(np.int64))


def test_dpsgd_validation_and_parsers():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.models import make_task

    for kw in ({"dp_clip": -1.0}, {"dp_clip": 1.0, "dp_sigma": -0.5}, {"dp_sigma": 1.0}):
        with pytest.raises(ValueError, match="dp_clip"):
            make_task("mnist", range(2), 2, "cpu", 0, **kw)
        with pytest.raises(ValueError, match="creditcard"):
            make_task("creditcard", range(2), 2, "cpu", 0, **kw)
    s = DP.shapes()[0]
    for clip, sigma, E, lr in ((0.0, 0.0, 1, 1.0), (1.0, -1.0, 1, 1.0), (1.0, 0.0, 65, 1.0), (1.0, 0.0, 1, 0.0)):
        with pytest.raises(ValueError):
            K.dpsgd_steps(*_args(s), clip, sigma, E, lr)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import prof_rounds
    for mod in (peer, fedsys, prof_rounds):
        ns = mod.build_parser().parse_args(["--dp-clip", "0.5", "--dp-sigma", "1.5"])
        assert (ns.dp_clip, ns.dp_sigma) == (0.5, 1.5)
        ns = mod.build_parser().parse_args([])
        assert (ns.dp_clip, ns.dp_sigma) == (0.0, 0.0)
