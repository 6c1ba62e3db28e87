"""The device signer against the host's batched signer on one box: a batch of verifier signatures from upload and
launch to the read-back (ops.schnorr.SchnorrSigner.sign, k_schnorr_sign) against rt().schnorr_sign_multi on
--threads host threads, alternating, on the same inputs; the bytes are compared first.

    python scripts/bench_sign.py [--sizes 16,210,2048] [--reps 200] [--threads 16] [-o out.json]

n = 210 is 3 verifiers x the 70-slot inbox of the 100-peer headline round.  One JSON line per size: the median, the
minimum and the 90th percentile of both, in us.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from biscotti_amd.native import rt  # noqa: E402
from biscotti_amd.ops.schnorr import SchnorrSigner  # noqa: E402


def _inputs(n: int, nkeys: int, seed: int):
    R = rt()
    order = R.bn256_order()
    rnd = random.Random(seed)
    nmsg = max(1, n // nkeys)   # every verifier signs the same workers' commitments
    msgs = [R.g1_base_mul(rnd.randrange(1, order)) for _ in range(nmsg)]
    sks = [rnd.randrange(1, order).to_bytes(32, "big") for _ in range(nkeys)]
    bases = [rnd.randbytes(32) for _ in range(nkeys)]
    mi = [i % nmsg for i in range(n)]
    ki = [(i // nmsg) % nkeys for i in range(n)]
    return msgs, sks, bases, mi, ki, list(mi)   # nonce id = the worker


def _stats(us: list) -> dict:
    us = sorted(us)
    return {"median_us": statistics.median(us), "min_us": us[0], "p90_us": us[int(0.9 * (len(us) - 1))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,210,2048")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sign needs a GPU")
    dev = torch.device("cuda", 0)
    R = rt()
    signer = SchnorrSigner(dev)
    lines = []
    for n in [int(s) for s in a.sizes.split(",")]:
        msgs, sks, bases, mi, ki, ids = _inputs(n, 3, n)
        msg_np = np.frombuffer(b"".join(msgs), np.uint8).reshape(-1, 64)
        msg_of = [msgs[m] for m in mi]

        def device():
            return signer.sign(msg_np, mi, ki, ids, sks, bases)()

        def host():
            return R.schnorr_sign_multi(msg_of, sks, ki, bases, ids, a.threads)

        sigs, status = device()
        want = host()
        assert not status.any() and [row.tobytes() for row in sigs] == [bytes(w) for w in want], "bytes differ"
        for _ in range(5):   # warm both
            device(), host()
        torch.cuda.synchronize()
        t_dev, t_host = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            device()
            t1 = time.perf_counter()
            host()
            t2 = time.perf_counter()
            t_dev.append(1e6 * (t1 - t0))
            t_host.append(1e6 * (t2 - t1))
        line = {"n": n, "reps": a.reps, "host_threads": a.threads, "device": _stats(t_dev), "host": _stats(t_host)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    signer.release()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
