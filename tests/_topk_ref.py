"""Top-k sparsification's reference, a stable sort by (key descending, index ascending), and the test rows."""
import numpy as np


def topk_ref(delta, qdelta, k):
    d, q = delta.copy(), qdelta.copy()
    for p in range(d.shape[0]):
        key = d[p].view(np.uint32) & np.uint32(0x7FFFFFFF)
        drop = np.lexsort((np.arange(key.size), -key.astype(np.int64)))[k:]
        d[p, drop], q[p, drop] = 0.0, 0
    return d, q


def rows(D, k):
    """fp32 [4, D] and its quantisation: normals; heavy ties (far more than r at the threshold, in every wave and
    chunk); fewer than k non-zeros; one magnitude under both signs (the kept set is exactly 0..k-1)."""
    rng = np.random.default_rng(1000 * D + k)
    few = np.zeros(D)
    few[rng.permutation(D)[:k // 2]] = rng.standard_normal(k // 2)
    d = np.stack([rng.standard_normal(D), rng.choice([0, 1e-3, -1e-3, 2e-3, -2e-3], D), few,
                  0.25 * rng.choice([-1.0, 1.0], D)]).astype(np.float32)
    return d, np.trunc(d.astype(np.float64) * 1e4).astype(np.int64)


def check(d, q, kept, d_ref, q_ref, k):
    """Byte equality with the reference (a selection: exact), kept = the rows' non-zero qdelta entries."""
    assert d.tobytes() == d_ref.tobytes() and q.tobytes() == q_ref.tobytes()
    if k < d.shape[1]:
        assert kept.tolist() == np.count_nonzero(q_ref, axis=1).tolist()
