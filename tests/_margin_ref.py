"""Reference and case list of the margin-loss local step (the SVM task): plain numpy fp64.

Nothing here runs torch, and of the code under test only K.minibatch_indices (which rows a peer draws) is used.  The
case list is _ml_ref.softmax_cases() with W multiplied by 4: at the unscaled W almost every hinge is active and the
inactive branch would go untested; at W * 4 the reference has 58-100 % of a case's hinges active.  The lists are
built once per process and never modified; tests/test_margin_cpu.py vets every case (torch fp64 autograd, the
discontinuity guard, the CPU path) before tests/test_gpu_margin.py takes it to k_margin_step.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import _ml_ref as R
from biscotti_amd.ops import ml as K

W_SCALE = 4.0
# a case is usable only if every hinge of the fp64 reference is at least this far from its kink: the fp32 logits
# differ from the fp64 ones by a few 1e-6 on these shapes, so no hinge can change side in fp32 (a condition on
# the cases, not a tolerance on the results)
Z_GUARD = 1e-3


def margin_step_ref(X, y, off, ntrain, pid, W, d_in, d_out, B, seed, iteration, max_norm=100.0, lo=-1):
    """fp64 local step of every peer under the multi-class margin loss: (delta [P, nparam], loss [P], z).
    z[s][j] = 1 - x[s][y_s] + x[s][j]; loss = mean over the Bq = min(B, n) rows of sum_{j != y} max(0, z) / C;
    G = 1 / (C Bq) where z > 0 (strictly), -(active count) / (C Bq) at the label; gradient clipped by
    max_norm / (norm + 1e-6), delta = -grad.  z: per peer the hinges [Bq, C - 1] without the label's column."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    Wt, bt = W[: d_out * d_in].reshape(d_out, d_in), W[d_out * d_in:]
    P = len(pid)
    delta = np.zeros((P, d_out * d_in + d_out))
    loss = np.zeros(P)
    zs = []
    for p in range(P):
        li = int(pid[p]) - lo if lo >= 0 else p
        n, o = int(ntrain[li]), int(off[li])
        idx = K.minibatch_indices(int(pid[p]), iteration, n, B, seed)
        Bq = min(B, n)
        assert len(idx) == Bq
        rows = [o + i for i in idx]
        xb = (X[rows] - 0.5) * 2.0
        lab = np.asarray(y)[rows].astype(np.int64)
        logits = xb @ Wt.T + bt
        r = np.arange(Bq)
        z = 1.0 - logits[r, lab][:, None] + logits
        other = np.ones_like(z, dtype=bool)
        other[r, lab] = False
        on = other & (z > 0)
        loss[p] = (np.where(on, z, 0.0).sum(1) / d_out).mean()
        g = on / (d_out * Bq)
        g[r, lab] = -on.sum(1) / (d_out * Bq)
        flat = np.concatenate([(g.T @ xb).reshape(-1), g.sum(0)])
        coef = max_norm / (np.sqrt((flat * flat).sum()) + 1e-6)
        if coef < 1:
            flat = flat * coef
        delta[p] = -flat
        zs.append(z[other].reshape(Bq, d_out - 1))
    return delta, loss, zs


@lru_cache(maxsize=None)
def margin_cases() -> tuple:
    return tuple(c._replace(W=c.W * W_SCALE) for c in R.softmax_cases())


def _ref(c: R.SmCase, max_norm=100.0):
    return margin_step_ref(c.X, c.y, c.off, c.nt, c.pid, c.W, c.d_in, c.d_out, c.B, c.seed, c.it, max_norm, lo=c.lo)


@lru_cache(maxsize=None)
def margin_refs() -> dict:
    return {c.name: _ref(c) for c in margin_cases()}


# ---------------------------------------------------------------------------- exact cases
D_IN, D_OUT, BATCH, N_ROWS = 17, 10, 10, 12
TIE_CLASS = 3


def _exact(name: str, b_c: float, one_label: bool) -> R.SmCase:
    """Two peers of N_ROWS rows, W = 0 except b[TIE_CLASS] = b_c; one_label: every row labelled TIE_CLASS."""
    g = R._rng("margin" + name)
    X = g.random((2 * N_ROWS, D_IN), dtype=np.float32)
    y = (np.full(2 * N_ROWS, TIE_CLASS) if one_label else g.integers(0, D_OUT, 2 * N_ROWS)).astype(np.int32)
    W = np.zeros(D_OUT * D_IN + D_OUT)
    W[D_OUT * D_IN + TIE_CLASS] = b_c
    return R.SmCase(name, X, y, np.asarray([0, N_ROWS], np.int64), np.asarray([N_ROWS, N_ROWS], np.int32),
                    np.asarray([3, 10], np.int32), W, D_IN, D_OUT, BATCH, R.SM_SEED, 5, -1)


@lru_cache(maxsize=None)
def genesis_case() -> R.SmCase:
    """W = 0: every logit is 0, every hinge z = 1 is active."""
    return _exact("genesis", 0.0, one_label=False)


def genesis_closed_form(c: R.SmCase):
    """(delta [P, nparam], loss) of the genesis case from G = 1 / (C Bq), G[y] = -(C - 1) / (C Bq): no logits, no
    hinges.  The gradient's norm is far below max_norm = 100, so nothing is clipped; loss = (C - 1) / C."""
    C, X = c.d_out, np.asarray(c.X, np.float64)
    out = []
    for p in range(len(c.pid)):
        idx = K.minibatch_indices(int(c.pid[p]), c.it, int(c.nt[p]), c.B, c.seed)
        rows = [int(c.off[p]) + i for i in idx]
        Bq = len(rows)
        g = np.full((Bq, C), 1.0 / (C * Bq))
        g[np.arange(Bq), c.y[rows]] = -(C - 1.0) / (C * Bq)
        xb = (X[rows] - 0.5) * 2.0
        out.append(-np.concatenate([(g.T @ xb).reshape(-1), g.sum(0)]))
    return np.stack(out), (C - 1.0) / C


@lru_cache(maxsize=None)
def tie_case() -> R.SmCase:
    """b[c] = 1 and every row labelled c: z = 1 - 1 + 0 == 0 exactly in fp32 and in fp64, and z > 0 is strict:
    nothing is active, so delta, qdelta and the loss are all zero."""
    return _exact("tie", 1.0, one_label=True)


@lru_cache(maxsize=None)
def satisfied_case() -> R.SmCase:
    """b[c] = 2: z = -1 everywhere, every margin satisfied; all zero like the tie."""
    return _exact("satisfied", 2.0, one_label=True)


CLIP_NORM = 0.05


@lru_cache(maxsize=None)
def clip_case():
    """One W * 4 case at max_norm = 0.05: (case, its reference at that max_norm); the gradient is scaled down."""
    c = next(s for s in margin_cases() if s.name == "n40_B10")
    return c, _ref(c, CLIP_NORM)
