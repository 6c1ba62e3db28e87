"""The engine's signature audit (RunConfig.sig_audit) without a GPU: every signature this rank's verifiers produce
goes through the host verifier where its batch is joined; the chain does not change.  tests/test_gpu_schnorr.py
holds the device path."""
import logging

import pytest

from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine

ROUNDS = 3


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def run_engine(audit: bool, tamper=None, device="cpu", comm=None, **kw):
    """(block hashes, stats, signed (verifier, slot) pairs the audit's seam saw, the audit's log lines)."""
    cfg = RunConfig(num_nodes=12, dataset="creditcard", seed=6, max_iterations=100, deterministic_time=True,
                    sig_audit=audit, device=device, **kw)
    eng = BiscottiEngine(cfg, comm) if comm is not None else BiscottiEngine(cfg)
    seen = []

    def seam(sig_np, it):   # the audit's own copy of the round's signature matrix [nv, ni, 64]
        seen.append(int(sig_np.any(axis=2).sum()))
        if tamper is not None:
            tamper(sig_np, it)

    lines = _Lines()
    eng.log.addHandler(lines)
    try:
        eng.sig_audit_tamper = seam
        hashes = [eng.run_round(remaining=ROUNDS - i).block_hash for i in range(ROUNDS)]
        eng.drain()
        return hashes, dict(eng.stats), sum(seen), [ln for ln in lines.lines if ln.startswith("Signature audit")]
    finally:
        eng.log.removeHandler(lines)
        eng.close()


@pytest.fixture(scope="module")
def chain_without_audit():
    hashes, stats, seen, lines = run_engine(False)
    assert "sig_audit_checked" not in stats and "sig_audit_failures" not in stats
    assert seen == 0 and not lines          # with the flag off the audit never runs
    assert len(set(hashes)) == ROUNDS
    return hashes


def test_cpu_engine_sig_audit_checks_every_signature_and_keeps_the_chain(chain_without_audit):
    hashes, stats, seen, lines = run_engine(True)
    assert seen >= ROUNDS                   # at least one accepted slot a round
    assert stats["sig_audit_checked"] == seen
    assert stats["sig_audit_failures"] == 0 and not lines
    assert hashes == chain_without_audit


def test_cpu_engine_sig_audit_counts_one_flipped_bit(chain_without_audit):
    done = []

    def flip(sig_np, it):   # one bit of the first signed slot of iteration 1, once
        if it == 1 and not done:
            v, j = [(int(a), int(b)) for a, b in zip(*sig_np.any(axis=2).nonzero())][0]
            sig_np[v, j, 40] ^= 1
            done.append((v, j))

    hashes, stats, seen, lines = run_engine(True, flip)
    assert done
    assert stats["sig_audit_checked"] == seen
    assert stats["sig_audit_failures"] == 1
    assert len(lines) == 1 and "iteration 1" in lines[0] and "verifier" in lines[0] and "worker" in lines[0]
    assert hashes == chain_without_audit
