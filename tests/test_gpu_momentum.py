"""k_momentum_steps (local steps under momentum, weight decay and a proximal term) on the GPU against the fp64 reference
of tests/_momentum_ref.py (cases vetted on the CPU path by tests/test_momentum_cpu.py), its launcher's limits, its
determinism, and the engine: the native pre-step must run the same steps."""
import numpy as np
import pytest
import torch

import _local_ref as LS
import _momentum_ref as M
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K
from test_gpu_local_steps import _chain, g

pytestmark = pytest.mark.gpu


def _run(s, E, lr, loss, max_norm, m, lam, mu):
    return K.momentum_steps(g(s.X), g(s.y), g(s.off), g(s.nt), g(s.pid), g(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, E,
                            lr, m, lam, mu, loss=loss, max_norm=max_norm, lo=s.lo)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_momentum_steps_match_fp64_reference(case):
    M.check(case, lambda *a: [o.cpu().numpy() for o in _run(*a)])


def _raw(loss, d_in, d_out, B, E, lr, m, lam, mu, out, vwork=None):
    X, y = torch.rand((4, max(d_in, 1))).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), g(np.asarray([4], np.int32)), g(np.asarray([0], np.int32))
    W = torch.zeros(max(d_in * d_out + d_out, 512), dtype=torch.float64).cuda()
    rc = hip().bsc_momentum_steps(loss, X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(),
                                  W.data_ptr(), d_in, d_out, B, 1, 7, 0, 100.0, 1e4, E, lr, m, lam, mu,
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                  None if vwork is None else vwork.data_ptr(), -1, None, 0, K._stream())
    torch.cuda.synchronize()
    return rc


def test_momentum_steps_launcher_limits():
    out = [torch.full((512,), 7, dtype=dt).cuda() for dt in (torch.float32, torch.int64, torch.float32)]
    ok, nan = (0, 8, 4, 4, 2, 1.0, 0.5, 0.1, 0.5), float("nan")   # loss, d_in, d_out, B, E, lr, m, lam, mu: one replaced
    bad = [ok[:k] + (v,) + ok[k + 1:] for k, v in ((6, 1.0), (6, -0.1), (6, nan), (7, -0.1), (7, nan), (8, -0.5), (8, nan),
                                                   (4, 0), (4, 65), (5, 0.0), (5, -1.0), (2, 17), (1, 0), (0, 2))]
    bad.append((0, 2730, 3, 4, 2, 1.0, 0.5, 0.0, 0.0))   # a velocity at nparam 8193 needs the workspace
    assert [_raw(*b, out) for b in bad] == [-1] * len(bad)
    assert all(bool((o == 7).all()) for o in out)                       # nothing was launched, nothing written
    ctx = hip().bsc_round_create(None, None, None, None, 50, 10, 3, 0, 1, 1e4)
    assert hip().bsc_round_task_momentum(ctx, 0.5, 0.0, 0.0, None) == -1     # before a bind
    bind = (*[None] * 6, 4, 10, 10, 1, 0, 100.0, 1e4, 0, None, None, None, 0, 512, None)   # d_in 4, d_out 10: d = 50
    assert hip().bsc_round_bind_task(ctx, *bind) == 0
    assert [hip().bsc_round_task_momentum(ctx, *v, None) for v in ((1.0, 0, 0), (0, nan, 0), (0, 0, -1.0), (0.9, 0.1, 0.5))] \
        == [-1, -1, -1, 0]
    hip().bsc_round_destroy(ctx)
    assert _raw(1, 8, 4, 4, 64, 1.0, 0.9, 0.1, 0.5, out) == 0           # E at its maximum, a and v in LDS
    assert bool((out[0][36:] == 7).all()) and bool((out[1][36:] == 7).all()) and not bool((out[0][:36] == 7).any())


@pytest.mark.parametrize("i", [5, 6], ids=["a_v_in_lds", "v_in_workspace"])
def test_momentum_steps_two_launches_give_the_same_bytes(i):
    s, max_norm, _ = LS.shapes()[i]
    a, b = (_run(s, 5, 0.1, "ce", max_norm, 0.5, 0.1, 0.5) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_engine_pipelined_chain_equals_unpipelined_chain_under_the_local_optimiser():
    kw = dict(local_steps=3, local_momentum=0.5, local_decay=1e-3, local_prox=0.1)
    piped, plain = _chain(**kw), _chain("no_pipeline", **kw)
    assert piped[1] and not plain[1]                                    # the two runs took the two step paths
    assert piped[0] == plain[0]


def test_engine_all_zero_is_the_default_chain_and_momentum_is_not():
    default = _chain()[0]
    assert default == _chain(local_momentum=0.0, local_decay=0.0, local_prox=0.0)[0]
    assert default[0] != _chain(local_momentum=0.9, local_steps=3)[0][0]
