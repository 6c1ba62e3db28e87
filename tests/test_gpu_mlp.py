"""k_mlp_step and k_mlp_eval against the fp64 reference (tests/_mlp_ref.py), and FedSys under the MLP on the GPU."""
import numpy as np
import pytest
import torch

import _mlp_ref as M
from _ml_ref import QSCALE, SM_SEED
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu


def c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", M.step_cases(), ids=lambda s: s.name)
def test_mlp_step(case):
    s = case
    d_ref, l_ref, coefs, z1s = M.step_refs()[s.name]
    # conditions on the inputs: no Z1 entry at a ReLU kink, the clip on or off as the case says
    assert min(float((np.abs(z) / np.abs(z).max(1, keepdims=True)).min()) for z in z1s) > 1e-3
    assert (coefs < 1).all() if s.clipped else (coefs > 1).all()
    d, q, l = K.mlp_step(c(s.X), c(s.y), c(s.off), c(s.nt), c(s.pid), c(s.W), s.d_in, s.H, s.d_out, s.B, SM_SEED, 5,
                         lo=s.lo)
    d, l = d.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    rtol, atol = s.tol
    print(s.name, "max |delta - ref|", np.abs(d - d_ref).max(), "max |loss - ref| / ref", (np.abs(l - l_ref) / l_ref).max())
    np.testing.assert_allclose(d, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    # exact: Go's int64(float64(delta) * 10^precision) of the kernel's own delta
    np.testing.assert_array_equal(q.cpu().numpy(), np.trunc(d * QSCALE).astype(np.int64))
    if s.dead >= 0:
        assert not d[:, s.dead * s.d_in:(s.dead + 1) * s.d_in].any() and not d[:, s.H * s.d_in + s.dead].any()
        assert d[:, :s.H * s.d_in].any()


@pytest.mark.parametrize("N", [1, 255, 257])
def test_mlp_eval_counts(N):
    X, y, W, pred, gap = M.eval_case(N)
    assert gap > 1e-4
    miss = pred != y
    for split in (0, N // 2, N):
        ea, eb = K.mlp_errors_async(c(X), c(y), split, c(W), X.shape[1], 48, 10)()
        assert (round(ea * split), round(eb * (N - split))) == (int(miss[:split].sum()), int(miss[split:].sum()))


def test_fedsys_mlp_gpu_follows_cpu():
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.fedsys import FedSysEngine

    errs = {}
    for dev in ("cpu", None):
        cfg = RunConfig(num_nodes=8, dataset="mnist", perc_samples=50, device=dev, seed=3)
        eng = FedSysEngine(cfg, None if dev else Comm(device=torch.device("cuda", 0)), model="mlp", hidden=32)
        assert eng.gpu == (dev is None)
        errs[dev or "cuda"] = [eng.run_round().test_error for _ in range(3)]
    one = 1.0 / eng.task.eval_split
    assert np.abs(np.subtract(errs["cpu"], errs["cuda"])).max() <= one * (1 + 1e-9), errs
