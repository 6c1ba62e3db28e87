"""k_local_steps (E local SGD steps per round) on the GPU against the fp64 reference of tests/_local_ref.py (cases vetted
on the CPU path by tests/test_local_steps_cpu.py), its launcher's limits, its determinism, and the engine: the native
pre-step must run the E steps too, or the pipelined chain differs from the unpipelined one."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import _local_ref as L
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(s, E, lr, loss, max_norm):
    return K.local_steps(g(s.X), g(s.y), g(s.off), g(s.nt), g(s.pid), g(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, E, lr,
                         loss=loss, max_norm=max_norm, lo=s.lo)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_local_steps_match_fp64_reference(case):
    i, loss, E, lr = case
    s, max_norm, _ = L.shapes()[i]
    d_ref, l_ref = L.ref(*case)
    d, q, l = _run(s, E, lr, loss, max_norm)
    d, l = d.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    rtol, atol = L.tol(s, E)
    print(L.case_id(case), "max |delta - ref| / tol", (np.abs(d - d_ref) / (atol + rtol * np.abs(d_ref))).max(),
          "max |loss - ref|", np.abs(l - l_ref).max())
    np.testing.assert_allclose(d, d_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q.cpu().numpy(), np.trunc(d * 1e4).astype(np.int64))


def _raw(loss, d_in, d_out, B, E, lr, out, ones=None, nones=0):
    X, y = torch.rand((4, max(d_in, 1))).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), g(np.asarray([4], np.int32)), g(np.asarray([0], np.int32))
    W = torch.zeros(512, dtype=torch.float64).cuda()
    rc = hip().bsc_local_steps(loss, X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(),
                               W.data_ptr(), d_in, d_out, B, 1, 7, 0, 100.0, 1e4, E, lr, out[0].data_ptr(),
                               out[1].data_ptr(), out[2].data_ptr(), -1, None if ones is None else ones.data_ptr(),
                               nones, K._stream())
    torch.cuda.synchronize()
    return rc


def test_local_steps_launcher_limits_and_ones():
    out = [torch.full((512,), 7, dtype=dt).cuda() for dt in (torch.float32, torch.int64, torch.float32)]
    bad = [(0, 0, 4, 4, 2, 1.0), (0, 8, 17, 4, 2, 1.0), (0, 8, 4, 17, 2, 1.0), (0, 8, 4, 4, 0, 1.0), (0, 8, 4, 4, 65, 1.0),
           (0, 8, 4, 4, 2, 0.0), (0, 8, 4, 4, 2, -1.0), (2, 8, 4, 4, 2, 1.0), (-1, 8, 4, 4, 2, 1.0)]
    assert [_raw(*b, out) for b in bad] == [-1] * len(bad)
    assert all(bool((o == 7).all()) for o in out)                       # nothing was launched, nothing written
    ones = torch.full((301,), -7, dtype=torch.int32).cuda()
    assert _raw(1, 8, 4, 4, 64, 1.0, out, ones, 300) == 0               # E at its maximum
    assert ones.cpu().tolist() == [1] * 300 + [-7]                      # more than one pass of the 256 threads
    assert bool((out[0][36:] == 7).all()) and bool((out[1][36:] == 7).all()) and not bool((out[0][:36] == 7).any())


@pytest.mark.parametrize("i", [5, 6], ids=["a_in_lds", "a_in_row"])
def test_local_steps_two_launches_give_the_same_bytes(i):
    s, max_norm, _ = L.shapes()[i]
    a, b = (_run(s, 5, 1.0, "ce", max_norm) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@lru_cache(maxsize=None)
def _chain(ablation="", **kw):
    """(the block hashes of four mnist rounds at 20 peers, whether the native pre-step ran the local step)."""
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(num_nodes=20, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True,
                    ablation=ablation)
    eng = BiscottiEngine(cfg, Comm(device=torch.device("cuda", 0)), **kw)
    hashes = [bytes(eng.run_round().block_hash) for _ in range(4)]
    eng.drain()
    native = eng._native is not None and eng._native.task is not None
    assert eng.fsm.chain.verify()[0] and len(set(hashes)) == 4
    eng.close()
    return hashes, native


def test_engine_pipelined_chain_equals_unpipelined_chain_at_three_local_steps():
    piped, plain = _chain(local_steps=3), _chain("no_pipeline", local_steps=3)
    assert piped[1] and not plain[1]                                    # the two runs took the two step paths
    assert piped[0] == plain[0]


def test_engine_one_local_step_is_the_default_chain_and_three_are_not():
    default = _chain()[0]
    assert default == _chain(local_steps=1)[0] and default[0] != _chain(local_steps=3)[0][0]
