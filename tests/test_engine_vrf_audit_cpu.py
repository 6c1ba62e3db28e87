"""The engine's VRF audit (RunConfig.vrf_audit) without a GPU: every proof goes through the host verifier, the
chain does not change.  tests/test_gpu_vrf_verify.py holds the device path."""
from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine

ROUNDS = 4


def _run(audit: bool):
    cfg = RunConfig(num_nodes=12, dataset="creditcard", seed=6, max_iterations=100, deterministic_time=True,
                    vrf_audit=audit, device="cpu")
    eng = BiscottiEngine(cfg)
    try:
        hashes = [eng.run_round().block_hash for _ in range(ROUNDS)]
        eng.drain()
        return hashes, dict(eng.stats)
    finally:
        eng.close()


def test_cpu_engine_vrf_audit_checks_every_proof_and_keeps_the_chain():
    off_hashes, off_stats = _run(False)
    on_hashes, on_stats = _run(True)
    assert "vrf_audit_checked" not in off_stats and "vrf_audit_failures" not in off_stats
    assert on_stats["vrf_audit_checked"] > 0
    # every round: a roles proof per live peer (12) and a noiser proof per local worker
    assert on_stats["vrf_audit_checked"] >= ROUNDS * 12
    assert on_stats["vrf_audit_failures"] == 0
    assert on_hashes == off_hashes and len(set(on_hashes)) == ROUNDS


def test_vrf_audit_flag():
    import argparse

    from biscotti_amd.protocol.config import add_framework_flags, add_reference_flags, config_from_args

    ap = argparse.ArgumentParser()
    add_reference_flags(ap)
    add_framework_flags(ap)
    assert not config_from_args(ap.parse_args([])).vrf_audit and not RunConfig().vrf_audit
    assert config_from_args(ap.parse_args(["--vrf-audit"])).vrf_audit
    assert config_from_args(ap.parse_args(["-pa", "10.0.0.1"])) == RunConfig()   # accepted, no field
