"""The chain audit's host backend (protocol/chain_audit.py) on hand-built chains (_chain_audit_cases.py): every
block's verdict and first offending update, the native array view of a chain, and the command line's exit codes."""
import numpy as np
import pytest

import _chain_audit_cases as C
from biscotti_amd.native import rt
from biscotti_amd.protocol.chain_audit import TOL, Status, audit_chain, w_max

D = 37
# chain indices:  1 first block after genesis (one update: signed values, a coefficient above 2^31), 2 empty,
# 3 three updates (the middle one all zeros: infinity bytes), 4 two updates that cancel, 5 one update
PLAN = [(1, "mixed"), (0, ""), (3, "zero3"), (2, "cancel"), (1, "mixed")]
ARGS = dict(one=3, many=3, empty=2, single_a=1, single_b=5)


@pytest.fixture(scope="module", params=[2, 5])
def setup(request):
    key = rt().CommitKey.generate(D, request.param)
    cases = C.secagg_cases(key, D, PLAN, **ARGS)
    cases.update(C.plain_cases(key, D, [1, 0, 2, 3], target=4, upd=1))
    return key, cases


NAMES = ["honest", "quantum", "half_quantum", "nan", "inf", "over_bound", "byte_flipped", "short_commitment",
         "exchanged", "empty_changed", "fedsys", "plain_honest", "plain_wrong_delta", "plain_bad_point",
         "plain_short_vector", "plain_range", "plain_model_step", "plain_unaccepted_added"]


@pytest.mark.parametrize("name", NAMES)
def test_verdicts(setup, name):
    key, cases = setup
    specs, status, first = cases[name]
    chain = C.build(specs, D)
    before = [bytes(chain.block(i).hash) for i in range(len(chain))]
    res = audit_chain(chain, key, precision=4, device="cpu")
    print(name, res.status, res.first)
    assert res.backend == "host" and res.hash_ok
    assert np.array_equal(res.status, status), (res.status, status)
    assert np.array_equal(res.first, first), (res.first, first)
    assert res.ok == (name in ("honest", "plain_honest", "fedsys"))
    assert [bytes(chain.block(i).hash) for i in range(len(chain))] == before   # the audit never changes the chain
    bad = np.flatnonzero(np.isin(status, [3, 4, 5, 6, 7]))
    assert res.first_failing == (int(bad[0]) if bad.size else None)
    assert sum(res.counts.values()) == len(chain)


def test_honest_chain_covers_the_edges(setup):
    """What the honest chain is meant to contain is really in it."""
    key, cases = setup
    specs = cases["honest"][0]
    step1 = np.rint(specs[0]["W"] * C.SCALE)
    assert step1.max() > 2 ** 31 and step1.min() < -2 ** 31
    assert specs[2]["ups"][1]["c"] == bytes(64)                      # the all-zero update: infinity bytes
    assert np.array_equal(specs[3]["W"], specs[2]["W"]) and len(specs[3]["ups"]) == 2   # a zero aggregate
    assert not specs[1]["ups"]


def test_bounds_are_the_derived_ones():
    """7 u M scale < TOL at M = w_max (the derivation at kernels/msm.hip k_chain_coeffs), and 2^26 with scale 10^4
    lies inside the bound."""
    for prec in (0, 4, 6):
        scale = 10.0 ** prec
        assert 7 * 2.0 ** -53 * w_max(scale) * scale < TOL
    assert w_max(1e4) > 2.0 ** 26 and TOL < 0.25


def test_largest_model_in_range_is_not_inexact():
    """A step applied at the edge of RANGE as the engine applies it (W + v / scale) is still recovered exactly."""
    key = rt().CommitKey.generate(D, 2)
    rng = np.random.default_rng(7)
    W0 = np.zeros(D)
    q0 = rng.integers(int(0.9 * w_max(C.SCALE) * C.SCALE), int(0.99 * w_max(C.SCALE) * C.SCALE), size=D)
    q0 = (q0 * rng.choice([-1, 1], size=D)).astype(np.int64)
    W1 = W0 + q0.astype(np.float64) / C.SCALE
    q1 = rng.integers(-9999, 9999, size=D).astype(np.int64)
    W2 = W1 + q1.astype(np.float64) / C.SCALE
    specs = [{"W": W1, "ups": [{"c": key.commit(q0, 0), "delta": None, "acc": True}]},
             {"W": W2, "ups": [{"c": key.commit(q1, 0), "delta": None, "acc": True}]}]
    res = audit_chain(C.build(specs, D), key, device="cpu")
    assert list(res.status) == [Status.EMPTY, Status.OK, Status.OK]


def test_hash_failure_is_reported_beside_the_verdicts(setup):
    key, cases = setup
    chain = C.build(cases["honest"][0], D)
    b = chain.block(2)
    b.timestamp = 77   # the stored hash no longer matches
    other = rt().Blockchain.with_genesis(D)
    for i in range(1, len(chain)):
        other.append(b if i == 2 else chain.block(i))
    res = audit_chain(other, key, device="cpu")
    assert not res.hash_ok and not res.ok and res.first_failing is None
    assert np.array_equal(res.status, cases["honest"][1])


def test_audit_arrays_view(setup):
    key, cases = setup
    a = C.build(cases["plain_honest"][0], D).audit_arrays(D, 1, 99)
    assert list(a["kind"]) == [2, 0, 2, 2] and list(a["offsets"]) == [0, 1, 1, 3, 6]
    assert a["models"].shape == (5, D) and a["commits"].shape == (6, 64) and a["plain_delta"].shape == (6, D)
    assert list(a["flags"]) == [7, 7, 7, 7, 7, 6] and list(a["plain_update"]) == list(range(6))
    s = C.build(cases["honest"][0], D).audit_arrays(D, 3, 5)
    assert s["first"] == 3 and list(s["kind"]) == [1, 1] and list(s["offsets"]) == [0, 3, 5]
    assert s["plain_delta"].shape == (0, D) and s["models"].shape == (3, D)


def test_marshaled_valid(rt):
    g = np.frombuffer(rt.g1_base_mul(12345), np.uint8)
    p = 65000549695646603732796438742359905742825358107623003571877145026864184071783
    x, y = int.from_bytes(g[:32].tobytes(), "big"), int.from_bytes(g[32:].tobytes(), "big")
    rows = [g.tobytes(), bytes(64), g.tobytes()[:63] + bytes([g[63] ^ 1])]
    if x + p < 2 ** 256:
        rows.append((x + p).to_bytes(32, "big") + y.to_bytes(32, "big"))
    if y + p < 2 ** 256:
        rows.append(x.to_bytes(32, "big") + (y + p).to_bytes(32, "big"))
    got = rt.g1_marshaled_valid(np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 64))
    assert list(got) == [1, 1, 0] + [0] * (len(rows) - 3)


def test_cli_exit_codes(tmp_path, capsys):
    from biscotti_amd import audit

    key = rt().CommitKey.generate(D, 2)   # the key the command line generates
    cases = C.secagg_cases(key, D, PLAN, **ARGS)
    good, bad = tmp_path / "good.chain", tmp_path / "bad.chain"
    C.build(cases["honest"][0], D).save(str(good))
    C.build(cases["byte_flipped"][0], D).save(str(bad))
    assert audit.main(["--chain-file", str(good), "--device", "cpu"]) == 0
    out = capsys.readouterr().out
    assert "no failing block" in out and "BAD_POINT" not in out
    assert audit.main(["--chain-file", str(bad), "--device", "cpu"]) == 1
    out = capsys.readouterr().out
    assert "block 3 (iteration 2): BAD_POINT at update 1" in out and "first failing block 3" in out
    assert audit.main(["--chain-file", str(good), "--device", "cpu", "-d", "creditcard"]) == 1   # 37 != 25


@pytest.mark.parametrize("secure_agg", [True, False], ids=["secagg", "plain"])
def test_engine_chain_on_the_host(secure_agg):
    """Chains the CPU engine builds (creditcard, d = 25) pass; peer.py's --audit-chain helper audits with the
    engine's own key and records the verdict."""
    from biscotti_amd import peer
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    eng = BiscottiEngine(RunConfig(num_nodes=6, dataset="creditcard", num_verifiers=1, num_miners=2, num_noisers=1,
                                   device="cpu", seed=7, deterministic_time=True, secure_agg=secure_agg))
    try:
        for _ in range(4):
            eng.run_round()
        res = peer._audit(eng)
        print(res.summary())
        assert res.backend == "host" and res.ok and eng.stats["chain_audit_ok"] == 1
        assert set(res.status.tolist()) <= {Status.OK, Status.EMPTY} and (res.status == Status.OK).any()
        kinds = eng.fsm.chain.audit_arrays(eng.d, 1, len(eng.fsm.chain))["kind"]
        assert (1 if secure_agg else 2) in kinds.tolist()
    finally:
        eng.close()
