"""k_topk_rows (top-k sparsified updates) on the GPU against the stable-sort reference of tests/_topk_ref.py byte
for byte, its launcher's edges, the task, and the engine: the native pre-step must sparsify too, or the pipelined
chain differs from the unpipelined one."""
import numpy as np
import pytest
import torch

import _topk_ref as T
from biscotti_amd.native import hip
from biscotti_amd.ops import ml as K

pytestmark = pytest.mark.gpu


def g(a):
    return torch.from_numpy(a).cuda()


# the last row whose keys fit LDS (TK_LDS_KEYS = 14336) and the first that streams; lfw's 17486 streams too
@pytest.mark.parametrize("D,k", [(1, 1), (63, 1), (64, 64), (65, 7), (257, 256), (7850, 785), (7850, 7849),
                                 (14336, 1433), (14337, 1433), (17486, 174)])
def test_topk_rows_matches_stable_sort(D, k):
    d, q = T.rows(D, k)
    dg, qg, kept = g(d), g(q), torch.full((4,), -1, dtype=torch.int32).cuda()
    K.topk_rows_(dg, qg, k, kept)
    T.check(dg.cpu().numpy(), qg.cpu().numpy(), kept.cpu(), *T.topk_ref(d, q, k), k)
    assert np.flatnonzero(dg[3].cpu().numpy()).tolist() == list(range(k))   # all keys equal: the first k by index


def test_topk_launcher_and_round_task_topk_edges():
    d, q = T.rows(65, 7)
    dg, qg = g(d), g(q)
    for k, rc in ((0, -1), (66, -1), (65, 0)):
        assert hip().bsc_topk_rows(dg.data_ptr(), qg.data_ptr(), 4, 65, k, None, K._stream()) == rc
        T.check(dg.cpu().numpy(), qg.cpu().numpy(), None, d, q, 65)   # untouched
    ctx = hip().bsc_round_create(None, None, None, None, 50, 10, 3, 0, 1, 1e4)
    assert hip().bsc_round_task_topk(ctx, 5) == -1                    # before a bind
    bind = (*[None] * 6, 4, 10, 10, 1, 0, 100.0, 1e4, 0, None, None, None, 0, 512, None)   # d_in 4, d_out 10: d = 50
    assert hip().bsc_round_bind_task(ctx, *bind) == 0
    assert [hip().bsc_round_task_topk(ctx, k) for k in (-1, 51, 50, 0)] == [-1, -1, 0, 0]
    hip().bsc_round_destroy(ctx)


@pytest.mark.parametrize("loss", ["ce", "margin"])
def test_task_step_is_the_sparsified_dense_step(loss):
    from biscotti_amd import data
    from biscotti_amd.models.tasks import SoftmaxTask

    fed = data.mnist_federation(6, seed=3, n_train=6000, n_test=1000)
    dense, sparse = (SoftmaxTask(range(6), 6, "cuda", 3, federation=fed, loss=loss, topk=t) for t in (1.0, 0.1))
    W = g(np.random.default_rng(5).normal(0, 0.05, dense.nparam))
    (d0, q0), (d1, q1) = (t.step(W, 7, list(range(6))) for t in (dense, sparse))
    assert (sparse.topk_k, dense.topk_k) == (785, 0) and int(torch.count_nonzero(q1, dim=1).max()) <= 785
    T.check(d1.cpu().numpy(), q1.cpu().numpy(), None, *T.topk_ref(d0.cpu().numpy(), q0.cpu().numpy(), 785), 7850)


def test_pipelined_chain_equals_unpipelined_chain_and_learns():
    """20 peers, 30 rounds at theta = 0.1: the pipelined run (native pre-step, bsc_round_prestep_slot) writes the
    unpipelined run's chain (the Python step), and ends below the genesis model's test error on the same rows."""
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    out = []
    for abl in ("", "no_pipeline"):
        cfg = RunConfig(num_nodes=20, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True,
                        ablation=abl)
        eng = BiscottiEngine(cfg, Comm(device=torch.device("cuda", 0)), topk=0.1)
        genesis = eng.task.evaluate(eng.W)["test_error"]
        hashes = [bytes(eng.run_round().block_hash) for _ in range(30)]
        eng.drain()
        final = eng.task.evaluate(eng.W)["test_error"]
        out.append((hashes, eng._native is not None and eng._native.task is not None))
        assert eng.fsm.chain.verify()[0]
        eng.close()
    print("top-k 0.1 test error: genesis", genesis, "after 30 rounds", final)
    assert out[0][1] and not out[1][1]     # the two runs did take the two step paths
    assert out[0][0] == out[1][0] and len(set(out[0][0])) == 30 and final < genesis
