"""The chain audit's device backend (kernels/msm.hip k_chain_coeffs, k_g1_unmarshal, k_block_commit_check around the
row MSM) against the host backend and the verdicts known by construction (_chain_audit_cases.py), at the shapes
where the kernels can break; the unmarshal kernel against marshal; and the audit of chains a running engine built.
"""
import numpy as np
import pytest
import torch

import _chain_audit_cases as C
from biscotti_amd.protocol.chain_audit import Status, audit_chain

pytestmark = pytest.mark.gpu

# d = 37: shorter than a wave, no multiple of poly.  Blocks of 1, 0, 2, 65, 130, 3 and 1 updates: no point, one lane,
# two, more than a wave, two strides per lane with a tree over all 64 lanes, a three-lane tree.
PLAN_37 = [(1, "mixed"), (0, ""), (2, "cancel"), (65, "sparse"), (130, "sparse"), (3, "zero3"), (1, "mixed")]
ARGS_37 = dict(one=4, many=5, empty=2, single_a=1, single_b=7, bad_idx=100)
# d = 1030: two slabs of the row MSM, the second with 6 coefficients
PLAN_1030 = [(1, "mixed"), (2, "cancel"), (0, ""), (3, "zero3"), (1, "mixed")]
ARGS_1030 = dict(one=1, many=4, empty=3, single_a=1, single_b=5)
NAMES = ["honest", "quantum", "half_quantum", "nan", "inf", "over_bound", "byte_flipped", "short_commitment",
         "exchanged", "empty_changed", "fedsys"]
PLAIN_NAMES = ["plain_honest", "plain_wrong_delta", "plain_bad_point", "plain_short_vector", "plain_range",
               "plain_model_step", "plain_unaccepted_added"]
_SETUPS = {}


def _setup(d):
    """(key, device engine, cases with the host backend's result) per model width, built once."""
    if d not in _SETUPS:
        from biscotti_amd.native import rt
        from biscotti_amd.ops import bn256 as B

        key = rt().CommitKey.generate(d, 5 if d == 37 else 2)
        eng = B.DeviceCommitEngine(key, 10, 21 if d == 37 else 3, b0=8)
        cases = C.secagg_cases(key, d, *((PLAN_37, ) if d == 37 else (PLAN_1030, )), **(ARGS_37 if d == 37 else ARGS_1030))
        cases.update(C.plain_cases(key, d, [1, 0, 2, 5], target=4, upd=3))
        host = {}
        for name, (specs, _, _) in cases.items():
            r = audit_chain(C.build(specs, d), key, device="cpu")
            host[name] = (r.status.copy(), r.first.copy())
        _SETUPS[d] = (key, eng, cases, host)
    return _SETUPS[d]


def _check(d, name, slab):
    key, eng, cases, host = _setup(d)
    specs, status, first = cases[name]
    res = audit_chain(C.build(specs, d), key, engine=eng, slab=slab)
    print(d, name, slab, res.status, res.first)
    assert res.backend == "device" and res.hash_ok
    assert np.array_equal(res.status, host[name][0]) and np.array_equal(res.first, host[name][1])
    assert np.array_equal(res.status, status) and np.array_equal(res.first, first)


@pytest.mark.parametrize("slab", [None, 3], ids=["slab-default", "slab3"])
@pytest.mark.parametrize("name", NAMES)
def test_secagg_verdicts_d37(name, slab):
    """Seven blocks; with slab = 3 they take three passes (3 + 3 + 1)."""
    _check(37, name, slab)


@pytest.mark.parametrize("name", NAMES)
def test_secagg_verdicts_d1030(name):
    _check(1030, name, 2)


@pytest.mark.parametrize("d,slab", [(37, None), (37, 2), (1030, 4)])
@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_plain_verdicts(name, d, slab):
    """Eight update rows; with slab = 2 they take four passes."""
    _check(d, name, slab)


def _random_points(rt, n, seed):
    rng = np.random.default_rng(seed)
    return [rt.g1_base_mul(int(k)) for k in rng.integers(1, 2 ** 62, size=n)]


def test_unmarshal_round_trips_marshal(rt):
    from biscotti_amd.ops import bn256 as B

    pts = _random_points(rt, 150, 3)
    pts[7] = pts[64] = pts[149] = bytes(64)   # infinity
    data = torch.from_numpy(np.frombuffer(b"".join(pts), np.uint8).reshape(-1, 64).copy()).cuda()
    aff, valid = B.g1_unmarshal(data)
    assert bool((valid == 1).all())
    want = np.concatenate([np.asarray(rt.g1_affine_mont_u32(p), np.uint32).reshape(1, 16) for p in pts])
    assert np.array_equal(aff.cpu().numpy().view(np.uint32), want)   # the host's Montgomery limbs; infinity = zeros
    one = torch.tensor(np.array([0xa1f76999, 0xe7a35393, 0xdf4a4a61, 0x11a4772e, 0x9e7b23de, 0x55901347, 0xb55c7806,
                                 0x704afe1c], np.uint32).view(np.int32)).cuda()
    jac = torch.cat([aff, one.repeat(len(pts), 1)], 1)
    jac[[7, 64, 149], 16:] = 0   # Z = 0
    assert torch.equal(B.marshal(jac), data)
    assert np.array_equal(rt.g1_marshal_jac_batch(jac.cpu().numpy().view(np.uint32)), data.cpu().numpy())


def test_unmarshal_rejects(rt):
    from biscotti_amd.ops import bn256 as B

    p = 65000549695646603732796438742359905742825358107623003571877145026864184071783
    g = _random_points(rt, 1, 11)[0]
    x, y = int.from_bytes(g[:32], "big"), int.from_bytes(g[32:], "big")
    enc = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")   # noqa: E731
    rows = [g, bytes(64), enc(x, p - y),                 # valid: the point, infinity, its negative
            enc(x, (y + 1) % p), enc((x + 1) % p, y),    # off the curve
            enc(p, y), enc(x, p), enc(0, 1), enc(2 ** 256 - 1, 2 ** 256 - 1), enc(p - 1, 0)]
    want = [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    if x + p < 2 ** 256:    # the same point to a decoder that reduces; refused here
        rows.append(enc(x + p, y))
        want.append(0)
    if y + p < 2 ** 256:
        rows.append(enc(x, y + p))
        want.append(0)
    data = torch.from_numpy(np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 64).copy()).cuda()
    aff, valid = B.g1_unmarshal(data)
    assert valid.cpu().tolist() == want
    assert list(rt.g1_marshaled_valid(data.cpu().numpy())) == want
    assert not aff[3:].any()   # an invalid point comes back as infinity
    pre = torch.ones(len(rows), dtype=torch.int32, device="cuda")
    pre[0] = 0
    assert B.g1_unmarshal(data, pre)[1].cpu().tolist() == [0] + want[1:]


def _engine(**kw):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    base = dict(num_nodes=10, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True)
    base.update(kw)
    return BiscottiEngine(RunConfig(**base), Comm(device=torch.device("cuda", 0)))


def _copy_with(rt, chain, b, edit):
    """A copy of the chain whose block b went through edit(BlockData) (its hash recomputed; the links break)."""
    out = rt.Blockchain.with_genesis(len(chain.block(0).data.global_w))
    for i in range(1, len(chain)):
        blk = chain.block(i)
        if i == b:
            bd = blk.data
            edit(bd)
            blk.data = bd
            blk.set_hash()
        out.append(blk)
    return out


def test_engine_chain_secure_aggregation(rt):
    eng = _engine()
    try:
        for _ in range(4):
            eng.run_round()
        chain, dev = eng.fsm.chain, eng.crypto.eng
        res = audit_chain(chain, engine=dev, precision=eng.cfg.precision)
        print(res.summary())
        assert res.ok and set(res.status.tolist()) <= {Status.OK, Status.EMPTY} and (res.status == Status.OK).any()
        key = rt.CommitKey.generate(eng.d, 2)
        host = audit_chain(chain, key, precision=eng.cfg.precision, device="cpu")
        assert np.array_equal(res.status, host.status) and np.array_equal(res.first, host.first)
        b = int(np.flatnonzero(res.status == Status.OK)[0])

        def edit(bd):
            w = np.array(bd.global_w)
            w[123] += 1e-4   # one quantum
            bd.global_w = w
        bad = audit_chain(_copy_with(rt, chain, b, edit), engine=dev, precision=eng.cfg.precision)
        want = res.status.copy()
        want[b] = Status.MISMATCH
        if b + 1 < len(want):
            want[b + 1] = Status.MISMATCH if res.status[b + 1] == Status.OK else Status.EMPTY_CHANGED
        assert np.array_equal(bad.status, want) and not bad.ok and not bad.hash_ok and bad.first_failing == b
    finally:
        eng.close()


def test_engine_chain_plain(rt):
    eng = _engine(secure_agg=False, num_nodes=12)   # with 10 peers and this seed the leader gets no update
    try:
        for _ in range(4):
            eng.run_round()
        chain, dev = eng.fsm.chain, eng.crypto.eng
        res = audit_chain(chain, engine=dev, precision=eng.cfg.precision)
        print(res.summary())
        assert res.ok and set(res.status.tolist()) <= {Status.OK, Status.EMPTY} and (res.status == Status.OK).any()
        b = int(np.flatnonzero(res.status == Status.OK)[-1])
        n = chain.block(b).data.n_deltas
        k = n - 1

        def edit(bd):
            ups = bd.deltas
            v = list(ups[k].delta)
            v[4321] += 2e-4   # two quanta
            ups[k].delta = v
            bd.deltas = ups
        bad = audit_chain(_copy_with(rt, chain, b, edit), engine=dev, precision=eng.cfg.precision)
        want = res.status.copy()
        want[b] = Status.MISMATCH
        assert np.array_equal(bad.status, want) and bad.first[b] == k and not bad.ok
    finally:
        eng.close()
