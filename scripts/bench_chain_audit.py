"""Time the chain audit (protocol/chain_audit.py) on a chain of the headline configuration.

  python scripts/bench_chain_audit.py --rounds 100 --save /tmp/chain100.bin --out result.json
      runs the headline engine (MNIST, 100 peers, deterministic time) for --rounds rounds, saves the chain, times
      the device backend with the engine's own tables (median of --reps, the first call apart as warm-up), then
      the host backend once (--no-host skips it)
  python scripts/bench_chain_audit.py --chain-file /tmp/chain100.bin --device-only --out result.json
      audits a saved chain with tables of its own (their build time reported apart): the form to put behind
      a kernel profiler for the row MSM's share of the device time

One JSON line on stdout (and in --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--peers", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain-file", default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from biscotti_amd.native import rt
    from biscotti_amd.protocol.chain_audit import audit_chain

    R = rt()
    out = {"peers": a.peers}
    eng = None
    if a.chain_file:
        from biscotti_amd.ops.bn256 import DeviceCommitEngine

        chain = R.Blockchain.load(a.chain_file)
        d = len(chain.block(0).data.global_w)
        key = R.CommitKey.generate(d, 2)
        t0 = time.perf_counter()
        dev = DeviceCommitEngine(key, 10, 21, "cuda")
        torch.cuda.synchronize()
        out["table_build_s"] = round(time.perf_counter() - t0, 3)
        out["table_bytes"], out["b0"] = dev.table_bytes(), dev.b0
    else:
        from biscotti_amd.parallel.comm import Comm
        from biscotti_amd.protocol.config import RunConfig
        from biscotti_amd.protocol.engine import BiscottiEngine

        cfg = RunConfig(num_nodes=a.peers, dataset="mnist", seed=0, max_iterations=10 ** 9, lazy_eval=True,
                        deterministic_time=True)
        t0 = time.perf_counter()
        eng = BiscottiEngine(cfg, Comm.init())
        out["engine_build_s"] = round(time.perf_counter() - t0, 3)
        for n in range(a.rounds):
            eng.run_round(last=n == a.rounds - 1)
        torch.cuda.synchronize()
        chain, dev, d = eng.fsm.chain, eng.crypto.eng, eng.d
        key = R.CommitKey.generate(d, 2)
        out["b0"] = dev.b0
        if a.save:
            chain.save(a.save)
    out["blocks"], out["d"] = len(chain), d
    walls, res = [], None
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        res = audit_chain(chain, engine=dev)
        walls.append(time.perf_counter() - t0)
    out["device_first_call_s"] = round(walls[0], 4)
    out["device_s"] = [round(w, 4) for w in walls[1:]]
    out["device_median_s"] = round(statistics.median(walls[1:]), 4)
    out["device_counts"], out["device_ok"] = res.counts, res.ok
    if not (a.device_only or a.no_host):
        t0 = time.perf_counter()
        host = audit_chain(chain, key, device="cpu")
        out["host_s"] = round(time.perf_counter() - t0, 3)
        out["host_equal_device"] = bool((host.status == res.status).all() and (host.first == res.first).all())
    if eng is not None:
        eng.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
