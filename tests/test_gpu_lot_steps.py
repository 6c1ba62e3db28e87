"""k_lot_steps (local steps on lots of up to 256 examples) on the GPU against the fp64 references that
tests/_lot_cases.py borrows (cases vetted on the CPU path by tests/test_lot_steps_cpu.py), its launcher's limits, its
determinism, and the engine: the native pre-step must run the same steps."""
import numpy as np
import pytest
import torch

import _lot_cases as LC
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K
from test_gpu_local_steps import _chain, g

pytestmark = pytest.mark.gpu


def _run(s, E, lr, loss, **kw):
    return K.lot_steps(g(s.X), g(s.y), g(s.off), g(s.nt), g(s.pid), g(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, E, lr,
                       loss=loss, lo=s.lo, **kw)


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_lot_steps_match_fp64_reference(case):
    LC.check(case, lambda *a, **kw: [o.cpu().numpy() for o in _run(*a, **kw)])


def _raw(loss, d_in, d_out, L, E, lr, clip, sigma, out, gwork=None, ones=None, nones=0):
    X, y = torch.rand((4, max(d_in, 1))).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    off, nt, pid = torch.zeros(1, dtype=torch.int64).cuda(), g(np.asarray([4], np.int32)), g(np.asarray([0], np.int32))
    W = torch.zeros(max(d_in * d_out + d_out, 512), dtype=torch.float64).cuda()
    rc = hip().bsc_lot_steps(loss, X.data_ptr(), y.data_ptr(), off.data_ptr(), nt.data_ptr(), pid.data_ptr(),
                             W.data_ptr(), d_in, d_out, L, 1, 7, 0, 100.0, 1e4, clip, sigma, E, lr, out[0].data_ptr(),
                             out[1].data_ptr(), out[2].data_ptr(), None if gwork is None else gwork.data_ptr(), -1,
                             None if ones is None else ones.data_ptr(), nones, K._stream())
    torch.cuda.synchronize()
    return rc


def test_lot_steps_launcher_limits_and_ones():
    out = [torch.full((512,), 7, dtype=dt).cuda() for dt in (torch.float32, torch.int64, torch.float32)]
    ok, nan = (0, 8, 4, 32, 2, 1.0, 1.0, 0.5), float("nan")   # loss, d_in, d_out, L, E, lr, clip, sigma: one replaced
    bad = [ok[:k] + (v,) + ok[k + 1:] for k, v in ((1, 0), (2, 17), (3, 0), (3, 257), (4, 0), (4, 65), (5, 0.0), (5, nan),
                                                   (6, 0.0), (6, -1.0), (6, nan), (7, -0.5), (7, nan), (0, 2), (0, -1))]
    bad.append((0, 2730, 3, 32, 2, 1.0, 0.0, 0.0))   # the mean's clip at nparam 8193 needs the workspace
    assert [_raw(*b, out) for b in bad] == [-1] * len(bad)
    assert all(bool((o == 7).all()) for o in out)                       # nothing was launched, nothing written
    ones = torch.full((301,), -7, dtype=torch.int32).cuda()
    for clip, sigma in ((1.0, 0.5), (0.0, 0.0)):                        # L and E at their maxima on a 4-row shard
        ones.fill_(-7)
        assert _raw(1, 8, 4, 256, 64, 1.0, clip, sigma, out, None, ones, 300) == 0
        assert ones.cpu().tolist() == [1] * 300 + [-7]                  # more than one pass of the 256 threads
        assert bool((out[0][36:] == 7).all()) and bool((out[1][36:] == 7).all()) and not bool((out[0][:36] == 7).any())


@pytest.mark.parametrize("name", ["lot256_lds", "lot48_row"])
def test_lot_steps_two_launches_give_the_same_bytes(name):
    a, b = (_run(LC.shapes()[name], 3, 0.5, "ce", clip=LC.clip_of(name, "ce"), sigma=1.5) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_engine_pipelined_chain_equals_unpipelined_chain_at_lot_32():
    kw = dict(lot_size=32, dp_clip=0.5, dp_sigma=0.5, local_steps=2)
    piped, plain = _chain(**kw), _chain("no_pipeline", **kw)
    assert piped[1] and not plain[1]                                    # the two runs took the two step paths
    assert piped[0] == plain[0]


def test_engine_no_lot_is_the_default_chain_and_a_lot_is_not():
    default = _chain()[0]
    assert default == _chain(lot_size=0)[0] and default[0] != _chain(lot_size=32)[0][0]
