"""The MLP's CPU paths against the fp64 reference, its FedSys wiring and the places that refuse it (no GPU)."""
import numpy as np
import pytest
import torch

import _mlp_ref as M
from _ml_ref import QSCALE, SM_SEED
from biscotti_amd.models import make_task
from biscotti_amd.ops import ml as K
from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine
from biscotti_amd.protocol.fedsys import FedSysEngine


def _cfg(**kw):
    return RunConfig(**{**dict(num_nodes=8, dataset="mnist", perc_samples=50, device="cpu", seed=3), **kw})


@pytest.mark.parametrize("name", ["din7_h48_c10_b10", "din797_h64_c10_b10_clip"])
def test_mlp_step_cpu_against_reference(name):
    s = next(c for c in M.step_cases() if c.name == name)
    d_ref, l_ref, _, _ = M.step_refs()[name]
    t = torch.from_numpy
    d, q, l = K.mlp_step(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.H, s.d_out, s.B, SM_SEED, 5,
                         lo=s.lo)
    d = d.numpy().astype(np.float64)
    np.testing.assert_allclose(d, d_ref, rtol=s.tol[0], atol=s.tol[1])
    np.testing.assert_allclose(l.numpy(), l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.numpy(), np.trunc(d * QSCALE).astype(np.int64))


def test_fedsys_trains_the_mlp_and_is_reproducible():
    eng = FedSysEngine(_cfg(), model="mlp", hidden=32)
    assert eng.d == eng.task.nparam == K.mlp_nparam(784, 32, 10) and eng.W.abs().sum() > 0
    errs = [eng.run_round().test_error for _ in range(20)]
    assert errs[-1] < errs[0], errs
    again = FedSysEngine(_cfg(), model="mlp", hidden=32)
    for _ in range(20):
        again.run_round()
    assert again.model_digest() == eng.model_digest() and len(eng.model_digest()) == 64


def test_mlp_is_refused_where_it_has_no_kernel():
    with pytest.raises(ValueError, match="creditcard"):
        make_task("creditcard", range(2), 2, "cpu", 0, model="mlp")
    with pytest.raises(ValueError, match="linear scorer only"):
        make_task("mnist", range(2), 2, "cpu", 0, model="mlp", local_steps=2)
    with pytest.raises(ValueError, match="multiple of 16"):
        make_task("mnist", range(2), 2, "cpu", 0, model="mlp", hidden=40)
    with pytest.raises(ValueError, match="FedSys only"):
        BiscottiEngine(_cfg(num_verifiers=3, num_miners=3, num_noisers=2), model="mlp")
