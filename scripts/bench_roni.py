"""RONI committee at the reference shape (3 verifiers, inbox of 70, minibatch of 10, 784 x 10): the per-candidate
loop (the engine's _verify arithmetic: one train_error per verifier for the base model and one per inbox row, each a
k_eval_error launch and a blocking read-back) against the batched committee (k_roni_counts: one launch, one
read-back).  Synchronised wall-clock per committee after warm-up, median over the repetitions.

    python scripts/bench_roni.py [--reps 30] [--warmup 5] [--out FILE] [--dataset mnist|creditcard]

--dataset creditcard is the logistic task at its reference shape (50 peers, 3 verifiers, inbox of 35, the 8999
validation rows of creditcard.csv x 25 features): the loop's train_error is a torch matmul, a compare, a sum and a
blocking read-back per (verifier, model); the committee is LogisticTask.roni_committee_async (k_logit_counts: each
distinct candidate scored once, one launch, one read-back).  There the two steps' accept matrices are compared bit
for bit (a digest over every repetition), not only their totals.

Each of the two measurements runs in a child process of its own under `timeout` and the second starts only if the
first ended cleanly; the last line printed is one JSON object with both medians and their ratio.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, NI, PEERS, SEED = 3, 70, 100, 1
CREDIT = {"verifiers": [3, 21, 44], "inbox": 35, "peers": 50}
STEP_TIMEOUT_S = 240


def _setup():
    import numpy as np
    import torch

    from biscotti_amd import data as D
    from biscotti_amd.models.tasks import SoftmaxTask

    dev = torch.device("cuda", 0)
    fed = D.mnist_federation(PEERS, seed=SEED, n_train=20000, n_test=2000)   # the shard size does not enter
    task = SoftmaxTask(range(PEERS), PEERS, dev, SEED, federation=fed)
    g = torch.Generator().manual_seed(SEED)
    W = (0.01 * torch.randn((task.nparam,), generator=g, dtype=torch.float64)).to(dev)
    U = (0.01 * torch.randn((PEERS, task.nparam), generator=g, dtype=torch.float32)).to(dev)   # the noised updates
    rng = np.random.default_rng(SEED)
    verifiers = [3, 41, 77]
    inboxes = [rng.permutation(PEERS)[:NI].tolist() for _ in range(V)]
    return task, W, U, verifiers, inboxes


def _loop(task, W, U, verifiers, inboxes, it):
    import torch

    from biscotti_amd.utils import h2d

    out = []
    for v, inbox in zip(verifiers, inboxes):
        X = U.index_select(0, h2d(inbox, torch.long, U.device))
        base = task.train_error(W, v, it)
        out.append([task.train_error(W + X[i].double(), v, it) - base <= 0.02 for i in range(len(inbox))])
    return out


def _batched(task, W, U, verifiers, inboxes, it):
    import numpy as np
    import torch

    from biscotti_amd.ops import ml as K
    from biscotti_amd.utils import h2d_many

    rows_np, nrows_np = task.roni_rows(verifiers, it)
    rows, nrows, cand = h2d_many([(rows_np, torch.int64), (nrows_np, torch.int32),
                                  (np.asarray(inboxes, np.int32), torch.int32)], U.device)
    counts = K.roni_committee_async(task.X, task.y, rows, nrows, W, U, cand, task.d_in, task.d_out)()
    return K.roni_accept(counts, nrows_np).tolist()


def _setup_credit():
    import numpy as np
    import torch

    from biscotti_amd.models.tasks import LogisticTask

    dev = torch.device("cuda", 0)
    peers = CREDIT["peers"]
    task = LogisticTask(range(peers), peers, dev, SEED)
    g = torch.Generator().manual_seed(SEED)
    W = (0.1 * torch.randn((task.nparam,), generator=g, dtype=torch.float64)).to(dev)
    # the noised updates: large enough that RONI rejects some of them
    U = (0.03 * torch.randn((peers, task.nparam), generator=g, dtype=torch.float32)).to(dev)
    rng = np.random.default_rng(SEED)
    inboxes = [rng.permutation(peers)[:CREDIT["inbox"]].tolist() for _ in CREDIT["verifiers"]]
    return task, W, U, CREDIT["verifiers"], inboxes


def _batched_credit(task, W, U, verifiers, inboxes, it):
    import numpy as np

    from biscotti_amd.ops import ml as K

    counts, nrows = task.roni_committee_async(W, U, np.asarray(inboxes, np.int32))()
    return K.roni_accept(counts, nrows).tolist()


def _step(name, reps, warmup, dataset="mnist"):
    import hashlib

    import torch

    fn = {"loop": _loop, "batched": _batched_credit if dataset == "creditcard" else _batched}[name]
    args = _setup_credit() if dataset == "creditcard" else _setup()
    for it in range(warmup):
        fn(*args, it)
    times, accepted = [], 0
    digest = hashlib.sha256()
    for it in range(warmup, warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = fn(*args, it)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        accepted += sum(map(sum, ok))
        digest.update(bytes(int(bool(b)) for row in ok for b in row))
    rec = {"step": name, "reps": reps, "median_ms": round(statistics.median(times), 4),
           "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "accepted": accepted}
    if dataset == "creditcard":
        rec["accept_sha256"] = digest.hexdigest()[:16]
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--dataset", choices=["mnist", "creditcard"], default="mnist")
    ap.add_argument("--step", choices=["loop", "batched"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 repetitions")
    if a.step:
        _step(a.step, a.reps, a.warmup, a.dataset)
        return
    res = {}
    for name in ("loop", "batched"):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                            "--step", name, "--reps", str(a.reps), "--warmup", str(a.warmup), "--dataset", a.dataset],
                           capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:   # nothing more is started on the device after a failed step
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"step {name} ended with status {r.returncode}")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["loop"]["accepted"] == res["batched"]["accepted"], res   # the same decisions on the same inputs
    if a.dataset == "creditcard":
        assert res["loop"]["accept_sha256"] == res["batched"]["accept_sha256"], res   # every accept bit, every rep
        assert 0 < res["loop"]["accepted"] < a.reps * len(CREDIT["verifiers"]) * CREDIT["inbox"], res
        shape = {"dataset": "creditcard", "verifiers": len(CREDIT["verifiers"]), "inbox": CREDIT["inbox"],
                 "peers": CREDIT["peers"], "rows": 8999, "features": 25}
    else:
        shape = {"verifiers": V, "inbox": NI, "batch": 10, "d_in": 784, "d_out": 10}
    out = {"shape": shape, "loop": res["loop"],
           "batched": res["batched"],
           "loop_over_batched": round(res["loop"]["median_ms"] / res["batched"]["median_ms"], 1)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
