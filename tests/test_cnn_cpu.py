"""The CNN's CPU paths against the fp64 reference and torch autograd, its FedSys wiring and the places that refuse it
(no GPU)."""
import numpy as np
import pytest
import torch

import _cnn_ref as C
from _ml_ref import QSCALE, SM_SEED
from biscotti_amd.models import make_task, zoo
from biscotti_amd.ops import ml as K
from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine
from biscotti_amd.protocol.fedsys import FedSysEngine


def _cfg(**kw):
    return RunConfig(**{**dict(num_nodes=8, dataset="mnist", perc_samples=50, device="cpu", seed=3), **kw})


@pytest.mark.parametrize("name", ["s3_c10_b10_lr", "s12_c2_b16_clip_lr"])
def test_cnn_step_cpu_against_reference(name):
    s = next(c for c in C.step_cases() if c.name == name)
    d_ref, l_ref = C.step_refs()[name][:2]
    t = torch.from_numpy
    d, q, l = K.cnn_step(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.S * s.S, s.d_out, s.B, SM_SEED, 5,
                         lo=s.lo, lr=s.lr)
    d = d.numpy().astype(np.float64)
    np.testing.assert_allclose(d, d_ref, rtol=s.tol[0], atol=s.tol[1])
    np.testing.assert_allclose(l.numpy(), l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.numpy(), np.trunc(d * QSCALE).astype(np.int64))


def test_cnn_parameter_order_is_the_torch_module_s():
    """At S = 28, one peer, no clip: the CPU path's raw gradient is autograd's of zoo.MNISTCNNModel, flattened."""
    g = C._rng("cnnorder")
    X = torch.from_numpy(g.random((10, 784), dtype=np.float32))
    y = torch.from_numpy(g.integers(0, 10, 10).astype(np.int32))
    W = K.cnn_init(784, 10, 7)
    W[400:416] = torch.from_numpy(g.standard_normal(16) * 0.1)   # a bias gradient that depends on the bias
    one = torch.tensor([0], dtype=torch.int64)
    d, _, l = K.cnn_step(X, y, one, torch.tensor([10], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), W, 784,
                         10, 10, SM_SEED, 5, max_norm=1e9)
    model = zoo.MNISTCNNModel()
    with torch.no_grad():
        for par, v in zip(model.parameters(), model.reshape(W)):
            par.copy_(v)
    loss = torch.nn.functional.cross_entropy(model((X - 0.5) / 0.5), y.long())
    loss.backward()
    np.testing.assert_allclose(-d[0].numpy(), zoo.flatten_grads(model), rtol=1e-4, atol=1e-6)
    assert abs(float(l[0]) - float(loss.detach())) < 1e-5


def test_fedsys_trains_the_cnn_and_is_reproducible():
    eng = FedSysEngine(_cfg(), model="mnist_cnn")
    assert eng.d == eng.task.nparam == K.cnn_nparam(784, 10) == 164266 and eng.W.abs().sum() > 0
    errs = [eng.run_round().test_error for _ in range(10)]
    assert errs[-1] < errs[0], errs
    again = FedSysEngine(_cfg(), model="mnist_cnn")
    for _ in range(10):
        again.run_round()
    assert again.model_digest() == eng.model_digest() and len(eng.model_digest()) == 64


def test_cnn_is_refused_where_it_has_no_kernel():
    for ds in ("lfw", "creditcard"):
        with pytest.raises(ValueError, match="mnist's"):
            make_task(ds, range(2), 2, "cpu", 0, model="mnist_cnn")
    for kw in (dict(topk=0.5), dict(local_steps=2), dict(dp_clip=1.0), dict(dp_sigma=1.0), dict(lot_size=32),
               dict(local_momentum=0.5), dict(local_decay=0.1), dict(local_prox=0.1)):
        with pytest.raises(ValueError, match="linear scorer only"):
            make_task("mnist", range(2), 2, "cpu", 0, model="mnist_cnn", **kw)
    with pytest.raises(ValueError, match="unsupported model"):
        make_task("mnist", range(2), 2, "cpu", 0, model="cnn")
    with pytest.raises(ValueError, match="FedSys only"):
        BiscottiEngine(_cfg(num_verifiers=3, num_miners=3, num_noisers=2), model="mnist_cnn")
    assert make_task("mnist", range(2), 2, "cpu", 0, model="mnist_cnn", local_lr=0.5).lr == 0.5
