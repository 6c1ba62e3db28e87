"""The Schnorr signer's case set (tests/_schnorr_sign_cases.py) against the host signer, and the engine.sign_device
switch where there is no GPU: accepted, the host signs, the chain is the same.  tests/test_gpu_schnorr_sign.py holds
the device path."""
import pytest

from _schnorr_sign_cases import DRAWS, EDGE_IDS, be32, cases, entropy

from biscotti_amd.native import rt

ROUNDS = 3


def test_integer_model_equals_the_host_signer_and_stays_under_the_draw_cap():
    cs = cases()
    R = rt()
    items, sks, bases, messages = cs["items"], cs["sks"], cs["bases"], cs["messages"]
    for it in items:
        want = R.schnorr_sign(messages[it.msg_idx], be32(sks[it.key_idx]), entropy(bases[it.key_idx], it.nonce_id))
        assert bytes(want) == it.sig, it
        assert 1 <= it.vdraws <= DRAWS and 1 <= it.cdraws <= DRAWS, it   # no case may end in status 3
        assert R.schnorr_verify(messages[it.msg_idx], R.g1_base_mul(sks[it.key_idx]), it.sig)


def test_case_set_holds_what_the_signer_tests_need():
    cs = cases()
    items, n = cs["items"], cs["order"]
    assert cs["sks"][-2:] == [1, n - 1] and len(cs["sks"]) == 10
    for ki in (8, 9):   # sk = 1 and sk = n - 1 under every edge nonce id
        assert {it.nonce_id for it in items if it.key_idx == ki} >= set(EDGE_IDS)
    assert max(it.vdraws for it in items) >= 3 and max(it.cdraws for it in items) >= 3
    assert sum(it.msg_idx == 5 for it in items) >= 10   # several items share one message
    assert len(items) >= 65                             # the largest batch of the device test


def test_multi_key_host_batch_equals_the_case_set():
    """The engine's host path (schnorr_sign_multi: bases and ids per item) gives the same bytes."""
    cs = cases()
    items = cs["items"]
    got = rt().schnorr_sign_multi([cs["messages"][it.msg_idx] for it in items], [be32(s) for s in cs["sks"]],
                                  [it.key_idx for it in items], cs["bases"],
                                  [it.nonce_id - (1 << 32) if it.nonce_id >= 1 << 31 else it.nonce_id for it in items], 2)
    assert [bytes(g) for g in got] == [it.sig for it in items]


def test_signer_needs_a_gpu():
    from biscotti_amd.ops.schnorr import SchnorrSigner

    with pytest.raises(RuntimeError):
        SchnorrSigner("cpu")


def test_peer_parser_accepts_device_sign():
    from biscotti_amd import peer
    from biscotti_amd.protocol.config import RunConfig, config_from_args

    ap = peer.build_parser()
    assert ap.parse_args(["--device-sign"]).device_sign is True
    ns = ap.parse_args([])
    assert ns.device_sign is False
    assert config_from_args(ns) == RunConfig()   # the switch is no RunConfig field


def _run(sign_device):
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(num_nodes=12, dataset="creditcard", seed=6, max_iterations=100, deterministic_time=True,
                    device="cpu")
    eng = BiscottiEngine(cfg)
    try:
        assert eng.sign_device is False
        if sign_device is not None:
            eng.sign_device = sign_device
        hashes = [eng.run_round(remaining=ROUNDS - i).block_hash for i in range(ROUNDS)]
        eng.drain()
        return hashes, dict(eng.stats), eng.last_signatures.copy()
    finally:
        eng.close()


def test_cpu_engine_accepts_the_switch_and_signs_on_the_host():
    off_hashes, off_stats, off_sigs = _run(None)
    assert not any(k.startswith("sign_") for k in off_stats)   # off: no stat key appears
    hashes, stats, sigs = _run(True)
    assert hashes == off_hashes and len(set(hashes)) == ROUNDS
    assert stats["sign_device"] == 0 and stats["sign_device_host"] == 0 and stats["sign_table_bytes"] == 0
    assert sigs.any() and (sigs == off_sigs).all()
    assert {k: v for k, v in stats.items() if not k.startswith("sign_")}.keys() == off_stats.keys()
