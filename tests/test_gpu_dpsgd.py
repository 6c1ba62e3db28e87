"""k_dpsgd_steps (DP-SGD local steps: per-example clip, noise on the clipped sum) on the GPU against the fp64 reference
of tests/_dpsgd_ref.py (cases vetted on the CPU path by tests/test_dpsgd_cpu.py), the sensitivity bound it exists for,
its launcher's limits, its determinism, and the engine: the native pre-step must run the same steps."""
import numpy as np
import pytest
import torch

import _dpsgd_ref as DP
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K
from test_gpu_local_steps import _chain, g

pytestmark = pytest.mark.gpu


def _run(s, C, S, E, lr, loss):
    return K.dpsgd_steps(g(s.X), g(s.y), g(s.off), g(s.nt), g(s.pid), g(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, C, S,
                         E, lr, loss=loss, lo=s.lo)


@pytest.mark.parametrize("case", DP.CASES, ids=DP.case_id)
def test_dpsgd_steps_match_fp64_reference(case):
    i, loss, E, lr, _, S = case
    s = DP.shapes()[i]
    d_ref, l_ref, bq, C = DP.ref(*case)
    d, q, l = _run(s, C, S, E, lr, loss)
    d, l = d.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    rtol, atol = DP.tol(s, E, lr, S, C, bq)
    norm = np.sqrt((d * d).sum(1))
    assert (np.abs(d - d_ref) <= atol + rtol * np.abs(d_ref)).all()
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.cpu().numpy(), np.trunc(d * 1e4).astype(np.int64))
    if (E, lr, S) == (1, 1.0, 0.0):     # the sensitivity bound: one step moves no peer further than C
        assert (norm <= C * (1 + 1e-5)).all()


def _raw(loss, d_in, d_out, B, E, lr, clip, sigma, out, ones=None, nones=0):
    X, y = torch.rand((4, max(d_in, 1))).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), g(np.asarray([4], np.int32)), g(np.asarray([0], np.int32))
    W = torch.zeros(512, dtype=torch.float64).cuda()
    rc = hip().bsc_dpsgd_steps(loss, X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(),
                               W.data_ptr(), d_in, d_out, B, 1, 7, 0, 1e4, clip, sigma, E, lr, out[0].data_ptr(),
                               out[1].data_ptr(), out[2].data_ptr(), -1, None if ones is None else ones.data_ptr(),
                               nones, K._stream())
    torch.cuda.synchronize()
    return rc


def test_dpsgd_launcher_limits_and_ones():
    out = [torch.full((512,), 7, dtype=dt).cuda() for dt in (torch.float32, torch.int64, torch.float32)]
    ok, nan = (0, 8, 4, 4, 2, 1.0, 1.0, 0.5), float("nan")   # loss, d_in, d_out, B, E, lr, clip, sigma: one replaced
    bad = [ok[:k] + (v,) + ok[k + 1:] for k, v in ((1, 0), (2, 17), (3, 17), (4, 0), (4, 65), (5, 0.0), (5, nan), (6, 0.0),
                                                   (6, -1.0), (6, nan), (7, -0.5), (7, nan), (0, 2), (0, -1))]
    assert [_raw(*b, out) for b in bad] == [-1] * len(bad)
    assert all(bool((o == 7).all()) for o in out)                       # nothing was launched, nothing written
    ones = torch.full((301,), -7, dtype=torch.int32).cuda()
    assert _raw(1, 8, 4, 4, 64, 1.0, 1.0, 0.5, out, ones, 300) == 0     # E at its maximum
    assert ones.cpu().tolist() == [1] * 300 + [-7]                      # more than one pass of the 256 threads
    assert bool((out[0][36:] == 7).all()) and bool((out[1][36:] == 7).all()) and not bool((out[0][:36] == 7).any())


@pytest.mark.parametrize("i", [4, 5], ids=["a_in_lds", "a_in_row"])
def test_dpsgd_two_launches_give_the_same_bytes(i):
    a, b = (_run(DP.shapes()[i], DP.clip_of(i, "ce", "mixed"), 1.5, 3, 0.5, "ce") for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_engine_pipelined_chain_equals_unpipelined_chain_under_dpsgd():
    kw = dict(dp_clip=0.5, dp_sigma=0.5, local_steps=2)
    piped, plain = _chain(**kw), _chain("no_pipeline", **kw)
    assert piped[1] and not plain[1]                                    # the two runs took the two step paths
    assert piped[0] == plain[0]


def test_engine_no_dp_clip_is_the_default_chain_and_a_clip_is_not():
    default = _chain()[0]
    assert default == _chain(dp_clip=0.0)[0] and default[0] != _chain(dp_clip=0.5)[0][0]
