"""k_cnn_step and k_cnn_eval against the fp64 reference (tests/_cnn_ref.py), and FedSys under the CNN on the GPU."""
import numpy as np
import pytest
import torch

import _cnn_ref as C
from _ml_ref import QSCALE, SM_SEED
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu


def c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", C.step_cases(), ids=lambda s: s.name)
def test_cnn_step(case):
    s = case
    d_ref, l_ref, coefs, _, zs = C.step_refs()[s.name]
    # conditions on the inputs: no pre-activation within the fp32 error of a ReLU kink, the clip on or off as the case says
    assert min(C.kink_margin(z, s.W) for z in zs) > 1
    assert (coefs < 1).all() if s.clipped else (coefs > 1).all()
    args = (c(s.X), c(s.y), c(s.off), c(s.nt), c(s.pid), c(s.W), s.S * s.S, s.d_out, s.B, SM_SEED, 5)
    d, q, l = (t.cpu().numpy() for t in K.cnn_step(*args, lo=s.lo, lr=s.lr))
    again = [t.cpu().numpy() for t in K.cnn_step(*args, lo=s.lo, lr=s.lr)]
    rtol, atol = s.tol
    d64 = d.astype(np.float64)
    print(s.name, "max |delta - ref|", np.abs(d64 - d_ref).max(), "max (|delta - ref| - rtol |ref|)",
          (np.abs(d64 - d_ref) - rtol * np.abs(d_ref)).max(), "max |loss - ref| / ref", (np.abs(l - l_ref) / l_ref).max())
    np.testing.assert_allclose(d64, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    # exact: Go's int64(float64(delta) * 10^precision) of the kernel's own delta
    np.testing.assert_array_equal(q, np.trunc(d64 * QSCALE).astype(np.int64))
    for a, b in zip((d, q, l), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [1, 17, 33])
def test_cnn_eval_counts(N):
    X, y, W, pred, gap = C.eval_case(N)
    assert gap > 1e-4
    miss = pred != y
    for split in (0, N // 2, N):
        ea, eb = K.cnn_errors_async(c(X), c(y), split, c(W), X.shape[1], 10)()
        assert (round(ea * split), round(eb * (N - split))) == (int(miss[:split].sum()), int(miss[split:].sum()))


def test_fedsys_cnn_gpu_follows_cpu():
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.fedsys import FedSysEngine

    errs = {}
    for dev in ("cpu", None):
        cfg = RunConfig(num_nodes=8, dataset="mnist", perc_samples=50, device=dev, seed=3)
        eng = FedSysEngine(cfg, None if dev else Comm(device=torch.device("cuda", 0)), model="mnist_cnn", local_lr=0.5)
        assert eng.gpu == (dev is None)
        errs[dev or "cuda"] = [eng.run_round().test_error for _ in range(3)]
    one = 1.0 / eng.task.eval_split
    assert np.abs(np.subtract(errs["cpu"], errs["cuda"])).max() <= one * (1 + 1e-9), errs
