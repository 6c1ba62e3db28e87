"""fp64 reference and case list of the local multi-step update (K.local_steps, k_local_steps): plain numpy; of the code
under test only K.minibatch_indices (which rows step e draws).  Data and one-step tolerances are tests/_ml_ref.py's."""
from functools import lru_cache

import numpy as np

import _ml_ref as R
from biscotti_amd.ops import ml as K

LOSSES, STEPS, RATES = ("ce", "margin"), (1, 2, 5), (1.0, 0.1)


def local_steps_ref(s, loss, E, lr, max_norm):
    """(delta [P, nparam], last-step loss [P], smallest |z| of a margin hinge, smallest | ||g_e|| - max_norm | /
    max_norm, the set of clip decisions met) of case s: a_{e+1} = a_e - lr min(1, max_norm / (||g_e|| + 1e-6)) g_e."""
    X, W, y = np.asarray(s.X, np.float64), np.asarray(s.W, np.float64), np.asarray(s.y)
    nw = s.d_out * s.d_in
    delta, lossv, zmin, gap, clips = np.zeros((len(s.pid), W.size)), np.zeros(len(s.pid)), np.inf, np.inf, set()
    for p, q in enumerate(s.pid):
        li = int(q) - s.lo if s.lo >= 0 else p
        a = np.zeros(W.size)
        for e in range(E):
            idx = K.minibatch_indices(int(q), s.it, int(s.nt[li]), s.B, s.seed, tag=0x5EED ^ (e << 16))
            rows = [int(s.off[li]) + i for i in idx]
            xb, lab, r = (X[rows] - 0.5) * 2.0, y[rows].astype(np.int64), np.arange(len(rows))
            w = W + a
            lg = xb @ w[:nw].reshape(s.d_out, s.d_in).T + w[nw:]
            if loss == "ce":
                m = lg.max(1, keepdims=True)
                ex = np.exp(lg - m)
                g = ex / ex.sum(1, keepdims=True)
                lossv[p] = (m[:, 0] + np.log(ex.sum(1)) - lg[r, lab]).mean()
                g[r, lab] -= 1.0
                g /= len(rows)
            else:
                z = 1.0 - lg[r, lab][:, None] + lg
                z[r, lab] = np.inf                      # the label's own column is no hinge
                zmin = min(zmin, np.abs(z).min())
                on = (z > 0) & np.isfinite(z)
                lossv[p] = (np.where(on, z, 0.0).sum(1) / s.d_out).mean()
                g = on / (s.d_out * len(rows))
                g[r, lab] = -on.sum(1) / (s.d_out * len(rows))
            flat = np.concatenate([(g.T @ xb).reshape(-1), g.sum(0)])
            nrm = np.sqrt((flat * flat).sum())
            gap = min(gap, abs(nrm - max_norm) / max_norm)
            clips.add(bool(max_norm / (nrm + 1e-6) < 1))
            a = a - lr * min(1.0, max_norm / (nrm + 1e-6)) * flat
        delta[p] = a
    return delta, lossv, zmin, gap, clips


@lru_cache(maxsize=None)
def shapes() -> tuple:
    """(case, max_norm, every step clips).  The staging tile is 256 features wide (255 / 256 / 257); the update stays
    in LDS up to 8192 parameters (16 x (511 + 1)) and in its row from 8193 (3 x (2730 + 1)).  The data names and the
    minibatch seeds were picked on the CPU until ref()'s conditions held for every loss, E and rate."""
    lo = 40
    return ((R._sm("ls_d3", [5, 5], 1, 3, 2), 100.0, False),
            (R._sm("ls_d17_short0", [3, 1, 40, 7], 10, 17, 10, pid=[lo + 3, lo + 0, lo + 1], lo=lo), 100.0, False),
            (R._sm("ls_d255", [20, 20], 16, 255, 16, seed=R.SM_SEED + 1), 100.0, False),
            (R._sm("ls_d256", [12, 12], 10, 256, 10, seed=R.SM_SEED + 3), 100.0, False),
            (R._sm("ls_d257_clip", [12, 12], 10, 257, 10, seed=R.SM_SEED + 6), 0.05, True),
            (R._sm("ls_lds_8192", [12, 1], 10, 511, 16), 100.0, False),
            (R._sm("ls_row_8193", [20, 3], 16, 2730, 3), 100.0, False),
            (R._sm("ls_row_clip", [12, 12], 10, 600, 16, seed=R.SM_SEED + 6), 0.05, True))


CASES = [(i, loss, E, lr) for i in range(len(shapes())) for loss in LOSSES for E in STEPS for lr in RATES]


def case_id(v):
    return f"{shapes()[v[0]][0].name}-{v[1]}-E{v[2]}-lr{v[3]}"


@lru_cache(maxsize=None)
def ref(i, loss, E, lr):
    """The case's reference, with the conditions on the inputs asserted from the reference alone: no margin hinge
    within 1e-3 of its kink, no gradient norm within 1e-3 max_norm of the clip threshold, all or no steps clipped."""
    s, max_norm, clipped = shapes()[i]
    delta, lossv, zmin, gap, clips = local_steps_ref(s, loss, E, lr, max_norm)
    assert zmin > 1e-3 and gap > 1e-3 and clips == {clipped}, (zmin, gap, clips)
    return delta, lossv


def tol(s, E):
    """E times the one-step tolerance of the same width: the steps' errors add to first order."""
    return E * s.tol[0], E * s.tol[1]
