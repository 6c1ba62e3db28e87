"""Plain numpy fp64 reference of the CNN step and logits (k_cnn_step / k_cnn_eval), and their case table.

The draw (K.minibatch_indices), the transform, the clip and the quantisation are _ml_ref.softmax_step_ref's; the
cases are built like its own (_ml_ref._rng) and never modified.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

from _ml_ref import SM_SEED, _rng
from biscotti_amd.ops import ml as K


def split(W, S, d_out):
    F = 16 * (S + 4) ** 2
    return W[:400].reshape(16, 25), W[400:416], W[416:416 + d_out * F].reshape(d_out, F), W[416 + d_out * F:]


def patches(xb, S):
    """[Bq, (S + 4)^2, 25]: every output position's 5 x 5 window of the images zero-padded by 4."""
    Q = S + 4
    xp = np.pad(xb.reshape(-1, S, S), ((0, 0), (4, 4), (4, 4)))
    return np.stack([xp[:, ky:ky + Q, kx:kx + Q].reshape(-1, Q * Q) for ky in range(5) for kx in range(5)], 2)


def cnn_logits_ref(X, W, S, d_out):
    """(logits [N, d_out], pre-activations [N, 16, (S + 4)^2]) of rows X under (x - 0.5) * 2."""
    Wc, bc, Wfc, bfc = split(np.asarray(W, np.float64), S, d_out)
    z = np.einsum("npt,ct->ncp", patches((np.asarray(X, np.float64) - 0.5) * 2.0, S), Wc) + bc[None, :, None]
    return np.maximum(z, 0.0).reshape(len(z), -1) @ Wfc.T + bfc, z


def cnn_step_ref(X, y, off, ntrain, pid, W, S, d_out, B, seed, iteration, lr=1.0, max_norm=100.0, lo=-1):
    """(delta [P, nparam], loss [P], clip coefficient [P], raw gradient [P, nparam], pre-activations per peer)."""
    W = np.asarray(W, np.float64)
    _, _, Wfc, _ = split(W, S, d_out)
    P = len(pid)
    delta, loss, coefs, grads, zs = np.zeros((P, W.size)), np.zeros(P), np.zeros(P), np.zeros((P, W.size)), []
    for p in range(P):
        li = int(pid[p]) - lo if lo >= 0 else p
        n, o = int(ntrain[li]), int(off[li])
        rows = [o + i for i in K.minibatch_indices(int(pid[p]), iteration, n, B, seed)]
        Bq = min(B, n)
        assert len(rows) == Bq
        lab = np.asarray(y)[rows].astype(np.int64)
        logits, z = cnn_logits_ref(np.asarray(X)[rows], W, S, d_out)
        a = np.maximum(z, 0.0).reshape(Bq, -1)
        m = logits.max(1, keepdims=True)
        e = np.exp(logits - m)
        se = e.sum(1, keepdims=True)
        r = np.arange(Bq)
        loss[p] = ((m[:, 0] + np.log(se[:, 0])) - logits[r, lab]).mean()
        g = e / se
        g[r, lab] -= 1.0
        g /= Bq
        dz = ((g @ Wfc) * (a > 0)).reshape(z.shape)
        dWc = np.einsum("ncp,npt->ct", dz, patches((np.asarray(X, np.float64)[rows] - 0.5) * 2.0, S))
        flat = np.concatenate([dWc.reshape(-1), dz.sum((0, 2)), (g.T @ a).reshape(-1), g.sum(0)])
        coefs[p] = max_norm / (np.sqrt((flat * flat).sum()) + 1e-6)
        grads[p] = flat
        delta[p] = -lr * flat * min(coefs[p], 1.0)
        zs.append(z)
    return delta, loss, coefs, grads, zs


def kink_margin(z, W):
    """min over the pre-activations of |z| / tau_c, tau_c = 32 * 2^-24 * (sum_taps |w_c| + |b_c|): the fp32 error bound
    of a 26-term dot with |x| <= 1.  Above 1: no ReLU of the fp32 kernels can differ from the reference's."""
    tau = 32 * 2.0 ** -24 * (np.abs(W[:400]).reshape(16, 25).sum(1) + np.abs(W[400:416]))
    return float((np.abs(z) / tau[None, :, None]).min())


class CnnCase(NamedTuple):
    name: str
    X: np.ndarray
    y: np.ndarray
    off: np.ndarray
    nt: np.ndarray
    pid: np.ndarray
    W: np.ndarray
    S: int
    d_out: int
    B: int
    lo: int
    lr: float
    clipped: bool   # the clip is active on every peer (False: on none)

    tol = (5e-4, 5e-6)   # the project's one-step tolerance for long sums against fp64 (_mlp_ref.MlpCase.tol)


def _case(name, S, d_out, B, ns=(12, 12), pid=None, lo=-1, lr=1.0, wscale=1.0, salt=0, clipped=False) -> CnnCase:
    g = _rng(f"cnn{name}/{salt}")   # salt: chosen once so that no pre-activation sits at a ReLU kink (kink_margin)
    ntot = int(sum(ns))
    X = g.random((ntot, S * S), dtype=np.float32)
    y = g.integers(0, d_out, ntot).astype(np.int32)
    off = (np.cumsum([0] + list(ns))[:-1]).astype(np.int64)
    pid = np.asarray(pid if pid is not None else [3 + 7 * i for i in range(len(ns))], np.int32)
    W = g.standard_normal(K.cnn_nparam(S * S, d_out)) * wscale
    W[:400] *= 0.2                                           # pre-activations of order 1
    W[416:416 + d_out * 16 * (S + 4) ** 2] *= 0.25 / (S + 4)   # logits of order 1 at every S
    return CnnCase(name, X, y, off, np.asarray(ns, np.int32), pid, W, S, d_out, B, lo, lr, clipped)


@lru_cache(maxsize=None)
def step_cases() -> tuple:
    lo = 40
    return (
        _case("s1_c2_b1", 1, 2, 1),
        _case("s3_c10_b10_lr", 3, 10, 10, lr=0.25),
        _case("s4_c16_b16", 4, 16, 16, ns=(16, 20)),
        _case("s4_c10_b10_clip", 4, 10, 10, wscale=40.0, clipped=True),
        _case("s12_c10_b10_short_lo", 12, 10, 10, ns=(3, 5, 12, 2, 9, 14), pid=[lo + 4, lo + 3], lo=lo,
              salt=2),
        _case("s12_c2_b16_clip_lr", 12, 2, 16, ns=(20, 20), lr=0.25, wscale=40.0, salt=1, clipped=True),
        _case("s28_c10_b16", 28, 10, 16, ns=(16,), salt=1),
    )


@lru_cache(maxsize=None)
def step_refs() -> dict:
    return {c.name: cnn_step_ref(c.X, c.y, c.off, c.nt, c.pid, c.W, c.S, c.d_out, c.B, SM_SEED, 5, lr=c.lr, lo=c.lo)
            for c in step_cases()}


@lru_cache(maxsize=None)
def eval_case(N: int, S: int = 5, d_out: int = 10):
    """(X fp32 [N, S^2], y, W, the reference's predicted class per row, its smallest top-two logit gap)."""
    g = _rng(f"cnneval{N}")
    X = g.random((N, S * S), dtype=np.float32)
    W = g.standard_normal(K.cnn_nparam(S * S, d_out)) * 0.3
    lg, _ = cnn_logits_ref(X, W, S, d_out)
    pred = lg.argmax(1)
    y = np.where(g.random(N) < 0.5, pred, (pred + 1) % d_out).astype(np.int32)   # about half the rows miss
    top = np.sort(lg, 1)
    return X, y, W, pred, float((top[:, -1] - top[:, -2]).min())
