"""Top-k sparsified updates without a GPU: K.topk_rows_'s CPU path against the stable-sort reference, the engine
with topk = 1 (off: today's chain), the validation and the CLIs."""
import pytest
import torch

import _topk_ref as T
from biscotti_amd.ops import ml as K


@pytest.mark.parametrize("D,k", [(1, 1), (65, 7), (257, 256), (7850, 785)])
def test_cpu_topk_rows_matches_stable_sort(D, k):
    d, q = T.rows(D, k)
    dt, qt, kept = torch.from_numpy(d.copy()), torch.from_numpy(q.copy()), torch.full((4,), -1, dtype=torch.int32)
    K.topk_rows_(dt, qt, k, kept)
    T.check(dt.numpy(), qt.numpy(), kept, *T.topk_ref(d, q, k), k)
    for bad in (0, D + 1):
        with pytest.raises(ValueError):
            K.topk_rows_(dt, qt, bad)


def _cfg(**kw):
    from biscotti_amd.protocol.config import RunConfig

    return RunConfig(num_nodes=12, seed=2, max_iterations=100, deterministic_time=True, device="cpu", **kw)


def test_topk_one_is_off_and_a_tenth_is_not():
    from biscotti_amd.protocol.engine import BiscottiEngine

    chains = []
    for kw in ({}, {"topk": 1.0}, {"topk": 0.1}):
        eng = BiscottiEngine(_cfg(dataset="mnist"), **kw)
        assert eng.task.topk_k == (785 if kw.get("topk") == 0.1 else 0) and eng.task.stateless_step
        chains.append([bytes(eng.run_round().block_hash) for _ in range(3)])
        assert eng.fsm.chain.verify()[0]
        eng.close()
    assert chains[0] == chains[1] != chains[2] and len(set(chains[0])) == 3


def test_topk_validation_and_parsers():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.models import make_task
    from biscotti_amd.protocol.fedsys import FedSysEngine

    for theta in (0.0, -0.1, 1.5, 1e-5):   # 1e-5 of 7850 entries: k < 1
        with pytest.raises(ValueError):
            make_task("mnist", range(2), 2, "cpu", 0, topk=theta)
    with pytest.raises(ValueError, match="creditcard"):
        make_task("creditcard", range(2), 2, "cpu", 0, topk=0.5)
    with pytest.raises(ValueError, match="creditcard"):
        FedSysEngine(_cfg(dataset="creditcard"), topk=0.5)
    for mod in (peer, fedsys):
        assert mod.build_parser().parse_args(["--topk", "0.25"]).topk == 0.25
        assert mod.build_parser().parse_args([]).topk == 1.0
