"""fp64 reference and case list of the DP-SGD local steps (K.dpsgd_steps, k_dpsgd_steps): plain numpy that materialises
every example's full gradient vector, takes its norm and clips it (no rank-one shortcut).  Of the code under test only
K.minibatch_indices and K.philox4x32; data, one-step tolerances and the fp64 Box-Muller are tests/_ml_ref.py's."""
from functools import lru_cache

import numpy as np

import _ml_ref as R
from biscotti_amd.ops import ml as K


def dpsgd_ref(s, loss, E, lr, C, S):
    """(delta [P, nparam], last-step loss [P], Bq [P], per-example norms by step, smallest |z| of a margin hinge)."""
    X, W, y = np.asarray(s.X, np.float64), np.asarray(s.W, np.float64), np.asarray(s.y)
    nw, P = s.d_out * s.d_in, len(s.pid)
    delta, lossv, bq, norms, zmin = np.zeros((P, W.size)), np.zeros(P), np.zeros(P), [[] for _ in range(E)], np.inf
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
                gam = ex / ex.sum(1, keepdims=True)
                lossv[p] = (m[:, 0] + np.log(ex.sum(1)) - lg[r, lab]).mean()
                gam[r, lab] -= 1.0
            else:
                z = 1.0 - lg[r, lab][:, None] + lg
                z[r, lab] = np.inf                      # the label's own column is no hinge
                zmin = min(zmin, np.abs(z).min())
                on = (z > 0) & np.isfinite(z)
                lossv[p] = (np.where(on, z, 0.0).sum(1) / s.d_out).mean()
                gam = on / s.d_out
                gam[r, lab] = -on.sum(1) / s.d_out
            tot = np.zeros(W.size)
            for i in r:                                 # one example's whole gradient, its norm, its clip
                g = np.concatenate([np.outer(gam[i], xb[i]).reshape(-1), gam[i]])
                n = np.sqrt((g * g).sum())
                norms[e].append(n)
                tot += min(1.0, C / (n + 1e-6)) * g
            if S > 0:
                c = K.philox4x32(np.arange(W.size), s.it, int(q), 0xD95D ^ (e << 16), s.seed & R.M32, s.seed >> 32)
                tot += S * C * R.gauss64(c[0], c[1])
            a = a - lr * tot / len(rows)
        delta[p], bq[p] = a, len(rows)
    return delta, lossv, bq, [np.asarray(v) for v in norms], zmin


@lru_cache(maxsize=None)
def shapes() -> tuple:
    """The staging tile is 256 features wide; the update stays in LDS up to 8192 parameters and in its row from 8193.
    The last is shape 0 with W scaled up until some margin rows have no active hinge (n_s = 0).  The data names were
    picked on the CPU until ref()'s conditions held for every case."""
    lo = 40
    idle = R._sm("dp_d3_a", [5, 5], 1, 3, 2)
    return (R._sm("dp_d3", [5, 5], 1, 3, 2),
            R._sm("dp_d17_short_a", [3, 1, 40, 7], 10, 17, 10, pid=[lo + 3, lo + 0, lo + 1], lo=lo),
            R._sm("dp_d255_g", [20, 20], 16, 255, 16), R._sm("dp_d257_c", [12, 12], 10, 257, 10),
            R._sm("dp_lds_8192_a", [12, 1], 10, 511, 16), R._sm("dp_row_8193_a", [20, 3], 16, 2730, 3),
            idle._replace(name="dp_d3_idle", W=idle.W * 10.0))


MODES = (("none", 0.0), ("all", 0.0), ("mixed", 0.0), ("mixed", 1.5))
CASES = [(i, loss, E, lr, mode, S) for i in range(6) for loss in ("ce", "margin") for E, lr in ((1, 1.0), (3, 0.5))
         for mode, S in MODES] + [(6, "margin", 3, 0.5, "none", 0.0)]


def case_id(v):
    return f"{shapes()[v[0]].name}-{v[1]}-E{v[2]}-lr{v[3]}-{v[4]}-S{v[5]}"


@lru_cache(maxsize=None)
def clip_of(i, loss, mode):   # C from the reference's step-0 per-example norms
    n0 = dpsgd_ref(shapes()[i], loss, 1, 1.0, np.inf, 0.0)[3][0]
    lo_, hi = n0[n0 > 0].min(), n0.max()
    return float({"none": 10.0 * hi, "all": 0.1 * lo_, "mixed": np.sqrt(lo_ * hi)}[mode])


@lru_cache(maxsize=None)
def ref(i, loss, E, lr, mode, S):
    """(delta, loss, Bq, C) of the case, with the conditions on the inputs asserted from the reference alone: no margin
    hinge within 1e-3 of its kink, no n_s within 1e-3 C of C at any step, and at step 0, whose norms C is taken from, one
    clip decision met in "none" / "all" and both in "mixed" (later steps may differ: a shard of one example that takes an
    all-clipped step of lr C fits that example and is no longer clipped)."""
    C = clip_of(i, loss, mode)
    delta, lossv, bq, norms, zmin = dpsgd_ref(shapes()[i], loss, E, lr, C, S)
    n = np.concatenate(norms)
    assert zmin > 1e-3 and np.abs(n - C).min() > 1e-3 * C, (zmin, np.abs(n - C).min() / C)
    assert {bool(C / (v + 1e-6) < 1) for v in norms[0]} == {"none": {False}, "all": {True}, "mixed": {False, True}}[mode]
    assert i != 6 or (n == 0).any()
    return delta, lossv, bq, C


def tol(s, E, lr, S, C, bq):
    """(rtol, atol [P, 1]): E one-step tolerances (the steps' errors add to first order) and, per draw, the project's
    bound of 1e-4 on a device N(0, 1) against the fp64 one, times what a draw moves an entry by."""
    return E * s.tol[0], E * s.tol[1] + (E * lr * S * C * 1e-4 / bq)[:, None]
