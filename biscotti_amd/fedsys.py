"""FedSys baseline entry point: ``python -m biscotti_amd.fedsys -i <k> -t <N> -d <dataset> [-ns 35 -rs -po]``.

Same launch modes as ``biscotti_amd.peer`` (one process per peer like FedSys/localTest.sh, or SPMD
under torchrun).  Flags and defaults follow FedSys/main.go:195-218: -ns 35, -rs, -po; EPSILON = 5
(main.go:42) for the creditcard at-source noise.  At exit rank 0 prints the final model digest and
iteration, the value FedSys/localTest.sh compares between peers.
"""
from __future__ import annotations

import argparse
import os
import sys

from .protocol.config import add_framework_flags, add_reference_flags, config_from_args


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="biscotti_amd.fedsys", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    add_reference_flags(ap)
    add_framework_flags(ap)
    ap.set_defaults(perc_samples=35, epsilon=5.0)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--model", default="softmax", choices=["softmax", "svm", "mlp", "mnist_cnn"],
                    help="softmax regression, svm: the same linear scorer under the multi-class margin loss, mlp: a "
                         "one-hidden-layer ReLU MLP under cross-entropy (k_mlp_step; the plain single step only) "
                         "(mnist and lfw), or mnist_cnn: the reference's Conv(1->16, 5x5) + ReLU + Linear CNN "
                         "(k_cnn_step; mnist only, the plain single step at rate --local-lr)")
    ap.add_argument("--mlp-hidden", type=int, default=32, metavar="H",
                    help="hidden units of --model mlp: a multiple of 16 in 16..64")
    ap.add_argument("--topk", type=float, default=1.0, metavar="THETA",
                    help="top-k sparsified updates: every worker keeps the int(d * THETA) largest-magnitude entries "
                         "of its update (mnist and lfw, 0 < THETA <= 1, 1 = off)")
    ap.add_argument("--local-steps", type=int, default=1, metavar="E",
                    help="local SGD steps per worker and round, each on a fresh minibatch (k_local_steps; mnist and "
                         "lfw, 1..64, 1 = the single step)")
    ap.add_argument("--local-lr", type=float, default=1.0, metavar="ETA", help="the rate of those local steps (> 0)")
    ap.add_argument("--dp-clip", type=float, default=0.0, metavar="C",
                    help="DP-SGD local steps (k_dpsgd_steps; mnist and lfw): clip each example's gradient to L2 norm C "
                         "before the minibatch is summed (0 = off)")
    ap.add_argument("--dp-sigma", type=float, default=0.0, metavar="S",
                    help="noise multiplier of those steps: N(0, (S C)^2) is added to the clipped sum (>= 0, needs --dp-clip)")
    ap.add_argument("--lot-size", type=int, default=0, metavar="L",
                    help="examples each local step draws, up to 256, in place of the batch size (k_lot_steps; mnist and "
                         "lfw, 0 = off)")
    ap.add_argument("--local-momentum", type=float, default=0.0, metavar="M",
                    help="heavy-ball momentum of the local steps, 0 <= M < 1 (k_momentum_steps; mnist and lfw, not with "
                         "--dp-clip or --lot-size; 0 = off)")
    ap.add_argument("--local-decay", type=float, default=0.0, metavar="LAMBDA",
                    help="weight decay of the local steps, >= 0")
    ap.add_argument("--local-prox", type=float, default=0.0, metavar="MU",
                    help="FedProx proximal weight of the local steps, >= 0")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    ns = ap.parse_args(argv)
    cfg = config_from_args(ns)
    if cfg.num_nodes <= 1 or not cfg.dataset:
        ap.print_usage()
        return 1
    if "WORLD_SIZE" not in os.environ and cfg.node_index >= 0:
        os.environ.update(WORLD_SIZE=str(cfg.num_nodes), RANK=str(cfg.node_index))
        os.environ.setdefault("LOCAL_RANK", "0")
        host, port = "127.0.0.1", "8000"
        if cfg.peers_file:
            with open(cfg.peers_file) as f:
                host, port = f.readline().strip().rsplit(":", 1)
        os.environ.setdefault("MASTER_ADDR", host)
        os.environ.setdefault("MASTER_PORT", port)
    from .parallel.comm import Comm
    from .protocol.fedsys import FedSysEngine

    comm = Comm.init(device=cfg.device)
    eng = FedSysEngine(cfg, comm, model=ns.model, topk=ns.topk, local_steps=ns.local_steps, local_lr=ns.local_lr,
                       dp_clip=ns.dp_clip, dp_sigma=ns.dp_sigma, lot_size=ns.lot_size, local_momentum=ns.local_momentum,
                       local_decay=ns.local_decay, local_prox=ns.local_prox, hidden=ns.mlp_hidden)
    n = 0
    while ns.rounds is None or n < ns.rounds:
        if eng.run_round() is None:
            eng.log.info("Reached the max iterations!")
            break
        n += 1
    if comm.rank == 0:
        sys.stdout.write(f"iteration {eng.iteration - 1} model {eng.model_digest()}\n")
        sys.stdout.flush()
    comm.barrier()
    comm.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
