"""Hand-built chains for the chain-audit tests (host backend: test_chain_audit_cpu.py; device backend:
test_gpu_chain_audit.py), with the verdict every block must get.

A chain is described by a list of block specs and built with fresh hashes, so a tampered chain still links and
hashes correctly: what the tests see is the audit's verdict, not Blockchain.verify()'s.

  spec = {"W": float64 [d], "ups": [{"c": 64 bytes or b"", "delta": float64 [d] or None, "acc": bool}, ...]}
"""
import copy

import numpy as np

from biscotti_amd.native import rt
from biscotti_amd.protocol.chain_audit import Status, w_max

SCALE = 1e4
OK, EMPTY, NO_COMMITMENTS, EMPTY_CHANGED, MISMATCH, BAD_POINT, INEXACT, RANGE = (int(s) for s in Status)


def build(specs, d):
    """Blockchain: genesis (zeros) + one block per spec, iteration = index - 1."""
    R = rt()
    chain = R.Blockchain.with_genesis(d)
    for it, s in enumerate(specs):
        bd = R.BlockData()
        bd.iteration = it
        bd.global_w = np.asarray(s["W"], np.float64)
        ups = []
        for k, u in enumerate(s["ups"]):
            x = R.Update()
            x.source_id, x.iteration, x.accepted = k, it, bool(u["acc"])
            x.commitment = bytes(u["c"])
            if u["delta"] is not None:
                x.delta = [float(v) for v in u["delta"]]
            ups.append(x)
        bd.deltas = ups
        b = R.Block()
        b.timestamp = 1000 + it if ups else 0
        b.data = bd
        b.prev_hash = chain.latest_hash()
        b.stake = {0: 10}
        b.set_hash()
        chain.append(b)
    ok, why = chain.verify()
    assert ok, why
    return chain


def _update_rows(rng, d, n, kind):
    """int64 [n, d] quantised updates.  kind: 'mixed' dense signed values with one coefficient above 2^31 and one
    below -2^31; 'zero3' three updates, the middle one all zeros (its commitment is the infinity bytes);
    'cancel' two updates that cancel; 'sparse' three nonzero coefficients per update (many updates, cheap to
    commit on the host)."""
    if kind == "cancel":
        q = rng.integers(-9000, 9000, size=(1, d))
        return np.concatenate([q, -q]).astype(np.int64)
    if kind == "sparse":
        q = np.zeros((n, d), np.int64)
        for r in range(n):
            q[r, rng.choice(d, size=3, replace=False)] = rng.integers(-20000, 20000, size=3)
        return q
    q = rng.integers(-9000, 9000, size=(n, d)).astype(np.int64)
    if kind == "zero3":
        q[1] = 0
    else:
        q[0, 1] = 3 * 2 ** 31 + 5
        q[0, d - 1] = -(2 ** 32) - 7
    return q


def secagg_specs(key, d, plan, seed=0):
    """An honest secure-aggregation chain: plan = [(number of updates, kind)], 0 updates = an empty block.  The
    model advances as the engine computes it: W + v / scale in fp64, v the integer aggregate."""
    rng = np.random.default_rng(seed)
    W = np.zeros(d)
    specs = []
    for n, kind in plan:
        if n == 0:
            specs.append({"W": W.copy(), "ups": []})
            continue
        q = _update_rows(rng, d, n, kind)
        W = W + q.sum(0).astype(np.float64) / SCALE
        specs.append({"W": W.copy(), "ups": [{"c": key.commit(q[r], 0), "delta": None, "acc": True}
                                             for r in range(q.shape[0])]})
    return specs


def plain_specs(key, d, counts, seed=1):
    """An honest plain chain (-sa false): every update carries its float32-valued delta, committed as
    trunc(delta * scale); the model is the previous one plus the accepted deltas, added in order.  The last update
    of a block with more than two is not accepted (and so not added)."""
    rng = np.random.default_rng(seed)
    W = np.zeros(d)
    specs = []
    for n in counts:
        ups = []
        for r in range(n):
            delta = (rng.standard_normal(d) * 0.3).astype(np.float32).astype(np.float64)
            acc = not (n > 2 and r == n - 1)
            ups.append({"c": key.commit((delta * SCALE).astype(np.int64), 0), "delta": delta, "acc": acc})
            if acc:
                W = W + delta
        specs.append({"W": W.copy(), "ups": ups})
    return specs


def expected_honest(specs):
    st = [EMPTY] + [OK if s["ups"] else EMPTY for s in specs]
    return np.array(st, np.int32), np.full(len(st), -1, np.int32)


def _flip(c: bytes, pos: int = 63) -> bytes:
    b = bytearray(c)
    b[pos] ^= 1
    return bytes(b)


def secagg_cases(key, d, plan, one, many, empty, single_a, single_b, bad_idx=1):
    """name -> (specs, status, first) for an honest chain and its tampered copies.  Block numbers (chain indices):
    `one` a block with updates whose successor has updates too, `many` a block with at least two updates, `empty`
    an empty block followed by a block with updates, single_a / single_b two blocks with one update each.  The
    byte_flipped case damages update bad_idx of block `many` and the block's last update: the first one counts."""
    base = secagg_specs(key, d, plan)
    st0, fi0 = expected_honest(base)
    cases = {"honest": (base, st0, fi0)}

    def case(name, mutate, changes):
        specs = copy.deepcopy(base)
        mutate(specs)
        st, fi = st0.copy(), fi0.copy()
        for b, (s, f) in changes.items():
            st[b], fi[b] = s, f
        cases[name] = (specs, st, fi)

    def bump(b, j, by):
        def m(specs):
            specs[b - 1]["W"][j] += by
        return m

    def put(b, j, v):
        def m(specs):
            specs[b - 1]["W"][j] = v
        return m

    both = lambda s: {one: (s, -1), one + 1: (s, -1)}   # noqa: E731
    case("quantum", bump(one, 2, 1.0 / SCALE), both(MISMATCH))
    case("half_quantum", bump(one, d - 1, 0.5 / SCALE), both(INEXACT))
    case("nan", put(one, 0, float("nan")), both(RANGE))
    case("inf", put(one, 3, float("inf")), both(RANGE))
    case("over_bound", put(one, 1, 2.0 * w_max(SCALE)), both(RANGE))

    def flip(specs):
        ups = specs[many - 1]["ups"]
        for u in {id(ups[bad_idx]): ups[bad_idx], id(ups[-1]): ups[-1]}.values():
            u["c"] = _flip(u["c"])
    case("byte_flipped", flip, {many: (BAD_POINT, bad_idx)})

    def short(specs):
        u = specs[many - 1]["ups"][0]
        u["c"] = u["c"][:63]
    case("short_commitment", short, {many: (BAD_POINT, 0)})

    def swap(specs):
        a, b = specs[single_a - 1]["ups"][0], specs[single_b - 1]["ups"][0]
        a["c"], b["c"] = b["c"], a["c"]
    case("exchanged", swap, {single_a: (MISMATCH, -1), single_b: (MISMATCH, -1)})
    case("empty_changed", bump(empty, 4, 1.0 / SCALE), {empty: (EMPTY_CHANGED, -1), empty + 1: (MISMATCH, -1)})

    def fedsys(specs):
        for u in specs[single_a - 1]["ups"]:
            u["c"], u["delta"] = b"", np.zeros(d)
    case("fedsys", fedsys, {single_a: (NO_COMMITMENTS, -1)})
    return cases


def plain_cases(key, d, counts, target, upd):
    """name -> (specs, status, first) for an honest plain chain and tampered copies of block `target` (at least
    three updates), update `upd`."""
    base = plain_specs(key, d, counts)
    st0, fi0 = expected_honest(base)
    cases = {"plain_honest": (base, st0, fi0)}

    def case(name, mutate, s, f):
        specs = copy.deepcopy(base)
        mutate(specs[target - 1])
        st, fi = st0.copy(), fi0.copy()
        st[target], fi[target] = s, f
        cases[name] = (specs, st, fi)

    def wrong_delta(s):
        s["ups"][upd]["delta"][5] += 2.0 / SCALE
    case("plain_wrong_delta", wrong_delta, MISMATCH, upd)

    def bad_point(s):
        s["ups"][upd]["c"] = _flip(s["ups"][upd]["c"], 31)
    case("plain_bad_point", bad_point, BAD_POINT, upd)

    def short_vec(s):
        s["ups"][upd]["delta"] = s["ups"][upd]["delta"][:d - 1]
    case("plain_short_vector", short_vec, MISMATCH, upd)

    def huge(s):
        s["ups"][upd]["delta"][0] = 1e300
    case("plain_range", huge, RANGE, upd)

    def step(s):
        s["W"][7] += 1e-9   # far below a quantum, far above the summation bound
    case("plain_model_step", step, MISMATCH, -1)

    def unaccepted_counted(s):   # the model also adds the update that was not accepted
        s["W"] = s["W"] + s["ups"][-1]["delta"]
    case("plain_unaccepted_added", unaccepted_counted, MISMATCH, -1)
    return cases
