"""Cases of the lot steps (K.lot_steps, k_lot_steps) for the CPU and the GPU tests.  There is no reference of its own:
the fp64 ones of tests/_local_ref.py (the mean's clip) and tests/_dpsgd_ref.py (per-example clip and noise) take any
s.B, here the lot L.  Data and one-step tolerances are tests/_ml_ref.py's, unscaled in L."""
from functools import lru_cache

import numpy as np

import _dpsgd_ref as DP
import _local_ref as LS
import _ml_ref as R

MODES = ("mean", "mean_clip", "dp", "dp_noise")   # max_norm 100 / 0.05; C "mixed" with S = 0 / 1.5


@lru_cache(maxsize=None)
def shapes() -> dict:
    """A row tile has 16 rows, a K tile 256 features; the update (and the step gradient) stay in LDS up to 8192
    parameters.  lot17: a tile and one row.  lot32_short: Lq = 32 (two tiles exactly), 20 (two tiles) and 1, pids out
    of order through lo.  lot33: a third tile of one row, a K tile of one feature.  lot48_row: nparam 8193, a and g in
    global memory.  lot256_lds: the largest lot, nparam 8192, one shard taken whole.  The data names and seeds were
    picked on the CPU until ref()'s conditions held for every case."""
    lo = 40
    return {"lot17": R._sm("lot17_a", [40, 40], 17, 17, 10),
            "lot32_short": R._sm("lot32_short_g", [20, 1, 64], 32, 255, 16, pid=[lo + 2, lo + 0, lo + 1], lo=lo,
                                 seed=R.SM_SEED + 12),
            "lot33": R._sm("lot33_e", [48, 48], 33, 257, 10, seed=R.SM_SEED + 15),
            "lot48_row": R._sm("lot48_row_b", [64, 3], 48, 2730, 3),
            "lot256_lds": R._sm("lot256_lds_a", [300, 256], 256, 511, 16, seed=R.SM_SEED + 2)}


CASES = [(name, loss, E, lr, mode) for name in shapes() for loss in ("ce", "margin") for E, lr in ((1, 1.0), (3, 0.5))
         for mode in MODES if (name, loss) != ("lot256_lds", "margin")]   # 256 x 16 hinges a step: some sit on a kink


def case_id(v):
    return f"{v[0]}-{v[1]}-E{v[2]}-lr{v[3]}-{v[4]}"


@lru_cache(maxsize=None)
def clip_of(name, loss):   # _dpsgd_ref.clip_of's "mixed": between the reference's smallest and largest step-0 norm
    n0 = DP.dpsgd_ref(shapes()[name], loss, 1, 1.0, np.inf, 0.0)[3][0]
    return float(np.sqrt(n0[n0 > 0].min() * n0.max()))


@lru_cache(maxsize=None)
def ref(name, loss, E, lr, mode):
    """(delta, loss, rtol, atol, K.lot_steps' keywords) of the case, with the conditions on the inputs asserted from
    the reference alone: no margin hinge within 1e-3 of its kink, no norm within 1e-3 (relative) of its threshold, and
    the intended clip decisions: of the mean at every step, per example (both kinds) at step 0."""
    s = shapes()[name]
    if mode in ("mean", "mean_clip"):
        max_norm = 0.05 if mode == "mean_clip" else 100.0
        delta, lossv, zmin, gap, clips = LS.local_steps_ref(s, loss, E, lr, max_norm)
        assert zmin > 1e-3 and gap > 1e-3 and clips == {mode == "mean_clip"}, (zmin, gap, clips)
        return delta, lossv, *LS.tol(s, E), {"max_norm": max_norm}
    C, S = clip_of(name, loss), 1.5 if mode == "dp_noise" else 0.0
    delta, lossv, bq, norms, zmin = DP.dpsgd_ref(s, loss, E, lr, C, S)
    n = np.concatenate(norms)
    assert zmin > 1e-3 and np.abs(n - C).min() > 1e-3 * C, (zmin, np.abs(n - C).min() / C)
    assert {bool(C / (v + 1e-6) < 1) for v in norms[0]} == {False, True}
    return delta, lossv, *DP.tol(s, E, lr, S, C, bq), {"clip": C, "sigma": S}


def check(case, run):
    """run(s, E, lr, loss, **keywords) -> K.lot_steps' (delta, qdelta, loss) as numpy arrays, against ref(case)."""
    name, loss, E, lr, mode = case
    d_ref, l_ref, rtol, atol, kw = ref(*case)
    d, q, l = run(shapes()[name], E, lr, loss, **kw)
    d, l = d.astype(np.float64), l.astype(np.float64)
    print(case_id(case), "max |delta - ref| / tol", (np.abs(d - d_ref) / (atol + rtol * np.abs(d_ref))).max(),
          "max |loss - ref|", np.abs(l - l_ref).max())
    assert (np.abs(d - d_ref) <= atol + rtol * np.abs(d_ref)).all()
    np.testing.assert_allclose(l, l_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(q, np.trunc(d * 1e4).astype(np.int64))
    if (mode, E, lr) == ("dp", 1, 1.0):     # the sensitivity bound: one step moves no peer further than C
        assert (np.sqrt((d * d).sum(1)) <= kw["clip"] * (1 + 1e-5)).all()
