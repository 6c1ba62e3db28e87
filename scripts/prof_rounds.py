"""cProfile of steady-state headline rounds only (the engine built and warmed outside the profile): which Python
functions and which torch / native calls hold the round's host thread.

    python scripts/prof_rounds.py [--warm 30] [--rounds 200] [--emulate-world N] [--device-sign] [--model svm]
                                  [--no-profile] [-o out.txt]

--emulate-world N profiles rank 0 of an N-rank job (bench.py --emulate-world: the collectives filled locally).
--device-sign sets engine.sign_device (the verifiers' signatures from k_schnorr_sign).  --model svm runs the rounds
with the margin-loss local step (k_margin_step) instead of k_softmax_step.  --no-profile times the same
rounds without cProfile.  The last line printed is one JSON summary: ms per round (wall), the round thread's CPU us
per round, the final drain's parts and the signer's stats.
"""
import argparse
import cProfile
import io
import json
import os
import pstats
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from biscotti_amd.parallel.comm import Comm  # noqa: E402
from biscotti_amd.protocol.config import RunConfig  # noqa: E402
from biscotti_amd.protocol.engine import BiscottiEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--emulate-world", type=int, default=0)
    ap.add_argument("--device-sign", action="store_true")
    ap.add_argument("--model", default="softmax", choices=["softmax", "svm"])
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    comm = Comm.emulated(a.emulate_world) if a.emulate_world > 1 else Comm.init()
    torch.set_num_threads(1)
    eng = BiscottiEngine(RunConfig(num_nodes=100, seed=0, max_iterations=10**9, host_threads=14, lazy_eval=True), comm,
                         model=a.model)
    eng.sign_device = a.device_sign
    for _ in range(a.warm):
        eng.run_round()
    torch.cuda.synchronize()
    pr = None if a.no_profile else cProfile.Profile()
    t0, c0 = time.perf_counter(), time.thread_time()
    if pr is not None:
        pr.enable()
    for _ in range(a.rounds):
        eng.run_round()
    if pr is not None:
        pr.disable()
    t1, c1 = time.perf_counter(), time.thread_time()
    torch.cuda.synchronize()
    eng.drain()
    if pr is not None:
        s = io.StringIO()
        st = pstats.Stats(pr, stream=s)
        st.sort_stats("tottime").print_stats(70)
        st.sort_stats("cumulative").print_stats(90)
        txt = s.getvalue()
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt)
        print(txt[:6000])
    summary = {"model": eng.model, "device_sign": a.device_sign, "profiled": pr is not None, "rounds": a.rounds,
               "ms_per_round": 1e3 * (t1 - t0) / a.rounds, "host_thread_us_per_round": 1e6 * (c1 - c0) / a.rounds,
               "drain_parts_ms": getattr(eng, "drain_parts_ms", None),
               "sign_stats": {k: v for k, v in eng.stats.items() if k.startswith("sign_")}}
    eng.close()   # (flushes the engine's log lines)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
