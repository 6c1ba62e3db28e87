"""Float64 numpy reference of the logistic miss counts (k_logit_counts / ops.ml.logit_counts) and the check that
makes an exact comparison with it meaningful.

Model 0 is W; model 1 + j is W[k] + float64(U[sel[j]][k]) per feature (a sel entry outside [0, n_cand) is W).  A row
counts as a miss when sign(x . w') != y, with sign(0) = 0.

A (row, model) is *decisive* when |z| > 1e-12 * sum_k |x_k w'_k|: a dot product of at most 32 float64 terms, summed
in any order and with or without FMA, errs by at most about 32 * 2^-53 = 3.6e-15 of that sum, so every
implementation gives a decisive row the same sign.  The threshold leaves a factor of ~280 on top.  A row whose terms
are all exactly zero (W = 0, an all-zero x) gives exactly 0 in every order.  Anything else is undecided and must not
occur in a test's input: `reference` asserts that.
"""
import numpy as np

DECISIVE = 1e-12


def models_of(W, U=None, sel=None):
    """float64 [M, D]: the models the kernel scores, formed as it forms them."""
    W = np.asarray(W, np.float64)
    models = [W]
    for c in ([] if sel is None else np.asarray(sel).tolist()):
        ok = U is not None and 0 <= c < len(U)
        models.append(W + np.asarray(U[c], np.float32).astype(np.float64) if ok else W)
    return np.stack(models)


def reference(X, y, split, W, U=None, sel=None):
    """counts int64 [M, 2] of the reference, after asserting that every (row, model) is decisive or exactly zero."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    Wm = models_of(W, U, sel)
    z = X @ Wm.T                                   # [N, M]
    mag = np.abs(X) @ np.abs(Wm).T                 # sum_k |x_k w'_k|
    undecided = (np.abs(z) <= DECISIVE * mag) & (mag != 0.0)
    assert not undecided.any(), f"{int(undecided.sum())} undecided (row, model) pairs: pick another seed"
    miss = np.where(mag == 0.0, 0.0, np.sign(z)) != y[:, None]
    return np.stack([miss[:split].sum(0), miss[split:].sum(0)], 1).astype(np.int64)


def min_margin(X, W, U=None, sel=None):
    """The smallest |z| / sum_k |x_k w'_k| over the (row, model) pairs that are not exactly zero (printed by tests)."""
    X = np.asarray(X, np.float64)
    Wm = models_of(W, U, sel)
    z, mag = X @ Wm.T, np.abs(X) @ np.abs(Wm).T
    nz = mag != 0.0
    return float((np.abs(z[nz]) / mag[nz]).min()) if nz.any() else float("inf")
