"""Momentum, weight decay and the proximal term of the local steps without a GPU: K.momentum_steps' torch fp32 path
against the fp64 reference of tests/_momentum_ref.py on the small cases (which vets the reference and its conditions),
the arguments, and a CPU engine run."""
import os
import sys

import pytest
import torch

import _momentum_ref as M
from biscotti_amd.ops import ml as K

t = torch.from_numpy
OPT = ["--local-momentum", "0.5", "--local-decay", "0.001", "--local-prox", "0.1"]


def _run(s, E, lr, loss, max_norm, m, lam, mu):
    out = K.momentum_steps(t(s.X), t(s.y), t(s.off), t(s.nt), t(s.pid), t(s.W), s.d_in, s.d_out, s.B, s.seed, s.it, E, lr,
                           m, lam, mu, loss=loss, max_norm=max_norm, lo=s.lo)
    return [o.numpy() for o in out]


@pytest.mark.parametrize("case", [c for c in M.CASES if c[0] in (0, 1, 4)], ids=M.case_id)
def test_cpu_momentum_steps_match_fp64_reference(case):
    M.check(case, _run)


def test_local_optimiser_validation_and_parsers():
    from biscotti_amd import fedsys, peer
    from biscotti_amd.models import make_task

    for kw in ({"local_momentum": 1.0}, {"local_momentum": -0.1}, {"local_momentum": float("nan")},
               {"local_decay": -1e-3}, {"local_prox": -0.5}, {"local_prox": float("inf")}):
        with pytest.raises(ValueError, match="local_"):
            make_task("mnist", range(2), 2, "cpu", 0, **kw)
    for kw in ({"local_momentum": 0.5}, {"local_decay": 0.1}, {"local_prox": 0.1}):
        with pytest.raises(ValueError, match="creditcard"):
            make_task("creditcard", range(2), 2, "cpu", 0, **kw)
        for other in ({"dp_clip": 1.0}, {"lot_size": 32}):
            with pytest.raises(ValueError, match="dp_clip or lot_size"):
                make_task("mnist", range(2), 2, "cpu", 0, **kw, **other)
    task = make_task("mnist", range(2), 2, "cpu", 0, model="svm", local_prox=0.1, local_steps=2, topk=0.5)
    assert (task.local_momentum, task.local_decay, task.local_prox, task.local_opt) == (0.0, 0.0, 0.1, True)
    assert not make_task("mnist", range(2), 2, "cpu", 0).local_opt
    assert K.momentum_workspace(3, 8192, 0.5, "cpu") is None and K.momentum_workspace(3, 8193, 0.0, "cpu") is None
    assert K.momentum_workspace(3, 8193, 0.5, "cpu").shape == (3, 8193)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import prof_rounds
    for mod in (peer, fedsys, prof_rounds):
        ns = mod.build_parser().parse_args(OPT)
        assert (ns.local_momentum, ns.local_decay, ns.local_prox) == (0.5, 0.001, 0.1)
        ns = mod.build_parser().parse_args([])
        assert (ns.local_momentum, ns.local_decay, ns.local_prox) == (0.0, 0.0, 0.0)


def test_cpu_engines_take_the_local_optimiser_and_keep_a_valid_chain():
    from biscotti_amd import peer
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine
    from biscotti_amd.protocol.fedsys import FedSysEngine

    ns = peer.build_parser().parse_args(OPT)
    kw = dict(local_momentum=ns.local_momentum, local_decay=ns.local_decay, local_prox=ns.local_prox, local_steps=3)
    cfg = RunConfig(num_nodes=12, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True, device="cpu")
    eng, plain = BiscottiEngine(cfg, **kw), BiscottiEngine(cfg, local_steps=3)
    assert (eng.task.local_momentum, eng.task.local_decay, eng.task.local_prox) == (0.5, 0.001, 0.1)
    hashes = [[bytes(e.run_round().block_hash) for _ in range(2)] for e in (eng, plain)]
    assert eng.fsm.chain.verify()[0] and hashes[0][0] != hashes[1][0]   # the rounds' steps are K.momentum_steps'
    fed = FedSysEngine(cfg, **kw)
    assert fed.task.local_opt and fed.run_round() is not None
