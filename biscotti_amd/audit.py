"""Chain audit from the command line: ``python -m biscotti_amd.audit --chain-file F [-d mnist|lfw|creditcard]
[--commit-key K] [--precision 4] [--device cpu]``.

Checks every block's model step against the commitments the block stores (protocol/chain_audit.py), prints one
line per block that is not OK or EMPTY and a summary.  The commitment key is K (commitKey.json) or the generated
key PK[i] = 2^i G1 the engine uses without one; its length is the dataset's model width, or the genesis block's
when no dataset is given.  Exit status 0 iff the chain's hashes verify and no block is MISMATCH, BAD_POINT,
INEXACT, RANGE or EMPTY_CHANGED.
"""
from __future__ import annotations

import argparse
import sys


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="biscotti_amd.audit", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chain-file", required=True)
    ap.add_argument("-d", "--dataset", default=None, choices=["mnist", "lfw", "creditcard"])
    ap.add_argument("--commit-key", default=None, help="commitKey.json (default: the generated key, s = 2)")
    ap.add_argument("--precision", type=int, default=4)
    ap.add_argument("--device", default=None, help="cpu for the host backend (default: the GPU when there is one)")
    ap.add_argument("--slab", type=int, default=None, help="rows per pass of the device backend")
    ns = ap.parse_args(argv)
    from .native import rt
    from .protocol.chain_audit import audit_chain

    R = rt()
    chain = R.Blockchain.load(ns.chain_file)
    if len(chain) == 0:
        print("chain audit: the file holds no block")
        return 1
    width = len(chain.block(0).data.global_w)
    if ns.dataset:
        from .data import dataset_dims

        d = dataset_dims(ns.dataset)[0]
        if d != width:
            print(f"chain audit: the chain's models have {width} parameters, {ns.dataset} has {d}")
            return 1
    else:
        d = width
    key = R.CommitKey.load(ns.commit_key, d) if ns.commit_key else R.CommitKey.generate(d, 2)
    res = audit_chain(chain, key, precision=ns.precision, device=ns.device, slab=ns.slab)
    for ln in res.lines():
        print(ln)
    print(res.summary())
    return 0 if res.ok else 1


if __name__ == "__main__":
    sys.exit(main())
