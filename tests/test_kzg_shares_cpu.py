"""--kzg-audit shares on the CPU path: verifySecret (K13, kyber.go:650-673) per worker update instead of per
aggregate -- the flag's new value, the engine's counts, the row seeds and one row against the share-by-share check."""
import argparse

import numpy as np
import torch

from biscotti_amd.ops.bn256 import kzg_row_seed
from biscotti_amd.protocol import config as C
from biscotti_amd.protocol.config import RunConfig
from biscotti_amd.protocol.engine import BiscottiEngine


def _cfg(**kw):
    base = dict(num_nodes=6, dataset="creditcard", num_verifiers=1, num_miners=1, num_noisers=1, noising=False,
                device="cpu", seed=7, deterministic_time=True)
    base.update(kw)
    return RunConfig(**base)


def _hashes(eng):
    return [bytes(eng.fsm.chain.block(i).hash) for i in range(len(eng.fsm.chain))]


def test_shares_is_a_valid_value():
    RunConfig(kzg_audit="shares").validate()


def test_cli_accepts_shares():
    ap = argparse.ArgumentParser()
    C.add_framework_flags(ap)
    assert ap.parse_args(["--kzg-audit", "shares"]).kzg_audit == "shares"


def test_row_seed_helper(rt):
    for seed in (0, 5, 2**63 + 12345):
        for i in (0, 1, 34, 70000):
            assert kzg_row_seed(seed, i) == rt.kzg_r(seed, 2**40 + i)
    assert kzg_row_seed(2**64 + 3, 2) == kzg_row_seed(3, 2)   # seeds are taken mod 2^64, as the device takes them


def test_engine_rounds_audit_every_update():
    """Every update of every non-empty block is checked once and passes; the chain is the unaudited run's."""
    eng = BiscottiEngine(_cfg(kzg_audit="shares"))
    off = BiscottiEngine(_cfg())
    try:
        res = [eng.run_round() for _ in range(4)]
        for _ in range(4):
            off.run_round()
        eng.drain()
        blocks = [r for r in res if not r.empty]
        assert len(blocks) >= 3
        assert eng.stats["kzg_checks"] == len(blocks)
        assert eng.stats["kzg_failures"] == 0
        assert eng.stats["kzg_share_checks"] == sum(len(r.node_list) for r in blocks) > 0
        assert eng.stats["kzg_share_failures"] == 0 and eng.kzg_share_blame == []
        assert eng.fsm.chain.verify()[0]
        assert _hashes(eng) == _hashes(off)
    finally:
        eng.close()
        off.close()


def test_row_verdicts_agree_with_verify_secrets_batch(rt):
    """Two rows through the engine's per-row host check: the honest one passes and every (chunk, point) of it passes
    verifySecret on its own; the other has one share value off by one -- exactly that share fails verifySecret and
    exactly that row is blamed."""
    eng = BiscottiEngine(_cfg(kzg_audit="shares"))
    try:
        T, nch, poly = eng.T, eng.nchunks, eng.cfg.poly_size
        q = torch.from_numpy(np.random.default_rng(3).integers(-10**6, 10**6, size=(2, eng.d), dtype=np.int64))
        pts, ys = eng.crypto.shares(q)
        ys = ys.clone()
        (ccols, _, ycols_t, _), xs, _, _ = eng._agg_index([0], {0: 0})
        npts, kb, jb = len(xs), nch - 1, 2
        ys[1, kb, int(ycols_t[jb])] += 1
        flat = pts.view(2, nch * (T + 1), eng.crypto.point_width)
        e = eng._kzg_host_rows(flat, ys, [0, 1], [40, 41], ccols, ycols_t, xs, 9)
        assert e["rows_done"] == (2, [41])
        g2, g2s = eng._kzg_g2
        for r in (0, 1):
            row = flat[r].numpy()
            ok = []
            for k in range(nch):   # verifySecret's base of chunk k is PK[poly * k] (the consistent form, Q9)
                Ck = bytes(row[k * (T + 1) + T])
                W = [bytes(row[k * (T + 1) + int(c)]) for c in ycols_t]
                y = [int(ys[r, k, int(c)]) for c in ycols_t]
                ok.append(rt.verify_secrets_batch([Ck] * npts, W, g2, g2s, list(xs), y, 2,
                                                  eng.crypto.key.point(poly * k)))
            bad = [(k, j) for k in range(nch) for j in range(npts) if not ok[k][j]]
            assert bad == ([] if r == 0 else [(kb, jb)])
    finally:
        eng.close()
