"""Plain numpy fp64 reference of the MLP step and miss counts (k_mlp_step / k_mlp_eval), and their case table.

The draw (K.minibatch_indices), the transform, the clip and delta = -gradient are _ml_ref.softmax_step_ref's; the
cases are built like its own (_ml_ref._rng) and never modified.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

from _ml_ref import SM_SEED, _rng
from biscotti_amd.ops import ml as K


def split(W, d_in, H, d_out):
    a, b, c = H * d_in, H * d_in + H, H * d_in + H + d_out * H
    return W[:a].reshape(H, d_in), W[a:b], W[b:c].reshape(d_out, H), W[c:]


def mlp_step_ref(X, y, off, ntrain, pid, W, d_in, H, d_out, B, seed, iteration, max_norm=100.0, lo=-1):
    """(delta [P, nparam], loss [P], clip coefficient [P], Z1 of every peer's minibatch)."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    W1, b1, W2, b2 = split(W, d_in, H, d_out)
    P = len(pid)
    delta, loss, coefs, z1s = np.zeros((P, W.size)), np.zeros(P), np.zeros(P), []
    for p in range(P):
        li = int(pid[p]) - lo if lo >= 0 else p
        n, o = int(ntrain[li]), int(off[li])
        rows = [o + i for i in K.minibatch_indices(int(pid[p]), iteration, n, B, seed)]
        Bq = min(B, n)
        assert len(rows) == Bq
        xb = (X[rows] - 0.5) * 2.0
        lab = np.asarray(y)[rows].astype(np.int64)
        z1 = xb @ W1.T + b1
        h = np.maximum(z1, 0.0)
        logits = h @ W2.T + b2
        m = logits.max(1, keepdims=True)
        e = np.exp(logits - m)
        se = e.sum(1, keepdims=True)
        r = np.arange(Bq)
        loss[p] = ((m[:, 0] + np.log(se[:, 0])) - logits[r, lab]).mean()
        g = e / se
        g[r, lab] -= 1.0
        g /= Bq
        dh = (g @ W2) * (z1 > 0)
        flat = np.concatenate([(dh.T @ xb).reshape(-1), dh.sum(0), (g.T @ h).reshape(-1), g.sum(0)])
        coefs[p] = max_norm / (np.sqrt((flat * flat).sum()) + 1e-6)
        delta[p] = -flat * min(coefs[p], 1.0)
        z1s.append(z1)
    return delta, loss, coefs, z1s


def mlp_logits_ref(X, W, d_in, H, d_out):
    W1, b1, W2, b2 = split(np.asarray(W, np.float64), d_in, H, d_out)
    return np.maximum((np.asarray(X, np.float64) - 0.5) * 2.0 @ W1.T + b1, 0.0) @ W2.T + b2


class MlpCase(NamedTuple):
    name: str
    X: np.ndarray
    y: np.ndarray
    off: np.ndarray
    nt: np.ndarray
    pid: np.ndarray
    W: np.ndarray
    d_in: int
    H: int
    d_out: int
    B: int
    lo: int
    clipped: bool   # the clip is active on every peer (False: on none)
    dead: int       # a hidden unit that no row activates, or -1

    @property
    def tol(self):
        """k_softmax_step's one-step tolerance against fp64 (_ml_ref.SmCase.tol), unchanged."""
        return (5e-4, 5e-6) if self.d_in > 1024 else (2e-4, 2e-6)


def _case(name, d_in, H, d_out, B, ns=(12, 12), pid=None, lo=-1, wscale=1.0, dead=-1, salt=0, clipped=False) -> MlpCase:
    g = _rng(f"mlp{name}/{salt}")   # salt: searched once so that no Z1 entry sits at a ReLU kink (min_kink_margin)
    ntot = int(sum(ns))
    X = g.random((ntot, d_in), dtype=np.float32)
    y = g.integers(0, d_out, ntot).astype(np.int32)
    off = (np.cumsum([0] + list(ns))[:-1]).astype(np.int64)
    pid = np.asarray(pid if pid is not None else [3 + 7 * i for i in range(len(ns))], np.int32)
    W = g.standard_normal(K.mlp_nparam(d_in, H, d_out)) * wscale
    W1, b1, _, _ = split(W, d_in, H, d_out)
    W1 *= 1.0 / np.sqrt(d_in)          # Z1 of order 1 at every d_in
    if dead >= 0:                      # |W1 x| <= sum |W1| < -b1: the unit never fires
        b1[dead] = -2.0 * np.abs(W1[dead]).sum() - 1.0
    return MlpCase(name, X, y, off, np.asarray(ns, np.int32), pid, W, d_in, H, d_out, B, lo, clipped, dead)


@lru_cache(maxsize=None)
def step_cases() -> tuple:
    lo = 40
    return (
        _case("din7_h16_c2_b1", 7, 16, 2, 1),
        _case("din7_h48_c10_b10", 7, 48, 10, 10, salt=1),
        _case("din64_h16_c10_b16", 64, 16, 10, 16, ns=(16, 20)),
        _case("din64_h64_c16_b10", 64, 64, 16, 10, salt=40),
        _case("din64_h48_c2_b16_clip", 64, 48, 2, 16, ns=(20, 20), wscale=30.0, salt=20, clipped=True),
        _case("din797_h16_c16_b10", 797, 16, 16, 10, salt=2),
        _case("din797_h48_c10_b1", 797, 48, 10, 1, salt=1, clipped=True),
        _case("din797_h64_c10_b10_clip", 797, 64, 10, 10, wscale=10.0, clipped=True),
        _case("din797_h64_c2_b16", 797, 64, 2, 16, ns=(16, 33), salt=75),
        _case("short_shard", 64, 48, 10, 10, ns=(3, 12), salt=1),
        _case("lo_two_peers", 797, 16, 10, 10, ns=(3, 5, 12, 2, 9, 14), pid=[lo + 4, lo + 2], lo=lo),
        _case("dead_unit", 64, 48, 10, 10, dead=17, salt=942),
        _case("din1500_h64_c10_b10", 1500, 64, 10, 10, salt=47),
    )


@lru_cache(maxsize=None)
def step_refs() -> dict:
    return {c.name: mlp_step_ref(c.X, c.y, c.off, c.nt, c.pid, c.W, c.d_in, c.H, c.d_out, c.B, SM_SEED, 5, lo=c.lo)
            for c in step_cases()}


@lru_cache(maxsize=None)
def eval_case(N: int, d_in: int = 37, H: int = 48, d_out: int = 10):
    """(X fp32 [N, d_in], y, W, the reference's predicted class per row, its smallest top-two logit gap)."""
    g = _rng(f"mlpeval{N}")
    X = g.random((N, d_in), dtype=np.float32)
    W = g.standard_normal(K.mlp_nparam(d_in, H, d_out))
    lg = mlp_logits_ref(X, W, d_in, H, d_out)
    pred = lg.argmax(1)
    y = np.where(g.random(N) < 0.5, pred, (pred + 1) % d_out).astype(np.int32)   # about half the rows miss
    top = np.sort(lg, 1)
    return X, y, W, pred, float((top[:, -1] - top[:, -2]).min())
