"""Lot steps without a GPU: K.lot_steps' CPU path (local_steps' / dpsgd_steps' with B = L) against the fp64 references
on the two small cases of tests/_lot_cases.py, which also vets their input conditions, and the arguments."""
import os
import sys

import pytest
import torch

import _lot_cases as LC
from biscotti_amd.ops import ml as K

t = torch.from_numpy


def _run(s, E, lr, loss, **kw):
    out = K.lot_steps(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, E, lr,
                      loss=loss, lo=s.lo, **kw)
    return [o.numpy() for o in out]


@pytest.mark.parametrize("case", [c for c in LC.CASES if c[0] in ("lot17", "lot32_short")], ids=LC.case_id)
def test_cpu_lot_steps_match_fp64_reference(case):
    LC.check(case, _run)


def test_lot_size_validation_and_parsers():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.models import make_task

    assert K.LOT_MAX == 256
    for bad in (257, -1, 1.5, True):
        with pytest.raises(ValueError, match="lot_size"):
            make_task("mnist", range(2), 2, "cpu", 0, lot_size=bad)
    with pytest.raises(ValueError, match="creditcard"):
        make_task("creditcard", range(2), 2, "cpu", 0, lot_size=32)
    task = make_task("mnist", range(2), 2, "cpu", 0, lot_size=32, dp_clip=0.5, local_steps=2)
    assert (task.lot_size, task.batch) == (32, 10)
    s = LC.shapes()["lot17"]
    for L, kw in ((0, {}), (257, {}), (17, {"E": 65}), (17, {"lr": 0.0}), (17, {"clip": -1.0}), (17, {"sigma": 1.0})):
        with pytest.raises(ValueError):
            K.lot_steps(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, L, s.seed, s.it, **kw)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import prof_rounds
    for mod in (peer, fedsys, prof_rounds):
        assert mod.build_parser().parse_args(["--lot-size", "64"]).lot_size == 64
        assert mod.build_parser().parse_args([]).lot_size == 0


def test_peer_and_fedsys_lot_size_reaches_the_task():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine
    from biscotti_amd.protocol.fedsys import FedSysEngine

    cfg = RunConfig(num_nodes=12, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True, device="cpu")
    for mod, engine in ((peer, BiscottiEngine), (fedsys, FedSysEngine)):
        eng = engine(cfg, lot_size=mod.build_parser().parse_args(["--lot-size", "48"]).lot_size)
        assert (eng.lot_size, eng.task.lot_size, eng.task.batch) == (48, 48, cfg.batch_size)
        assert eng.run_round() is not None     # the round's steps are K.lot_steps'
        assert engine(cfg).task.lot_size == 0
