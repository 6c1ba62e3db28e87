"""Chain audit: each block's model step against the commitments the block stores (not in the reference, whose
verifyBlock is `return true`, DistSys/blockchain.go:61-64).

Every block carries the 64-byte polynomial commitment of each update that went into it.  The commitments add up
homomorphically, so anyone holding a chain and the commitment key can check that the model of block b is the model
of block b - 1 plus exactly the committed updates.  With scale = 10^precision and prev = global_w of block b - 1:

  empty block (no deltas)     global_w == prev bit for bit: EMPTY, else EMPTY_CHANGED.
  secure-aggregation block    (commitments, no delta vectors)  c_i = rint((W_b[i] - prev[i]) * scale) as int64;
                              OK iff sum_i c_i PK[i] == the G1 sum of the block's commitments.  Guards, each
                              ending the block's check, in this order: RANGE (a value that is not finite or
                              |W| > w_max(scale), in either model), INEXACT (|x scale - rint(x scale)| > TOL),
                              BAD_POINT (a commitment that is not 64 bytes, has a coordinate >= p, or is off
                              y^2 = x^3 + 3; all zeros is infinity; first = the first such update), MISMATCH.
  plain block                 (-sa false: deltas carry their vectors)  per update, in order, the commitment of
                              trunc(delta[i] * scale) (the engine's quantize) must equal the update's own:
                              the first update that fails gives the block BAD_POINT, RANGE (a value whose
                              quantum leaves int64) or MISMATCH with its index.  Then W_b - prev against the sum
                              of `delta` over the accepted updates (what the engine and createBlock,
                              DistSys/honest.go:361-371, add): MISMATCH with first = -1 when a coordinate
                              differs by more than (n + 2) 2^-52 (|prev| + sum |delta|), the bound of two
                              n-term fp64 summations in any order (the engine's and this one's, each within
                              n 2^-53 of the exact sum relative to the terms' magnitudes, plus higher orders).
  no commitment at all        (FedSys chains) NO_COMMITMENTS: never a failure.

TOL and w_max come from the fp64 error of fl(W + v / scale) - W, derived at kernels/msm.hip k_chain_coeffs:
within |W| <= 2^40 / scale the residual stays under 7 * 2^-13 < TOL = 2^-10 quanta, so a chain the engine
produced is never INEXACT inside RANGE.

Two backends with identical verdicts: the device one (ops/bn256.py DeviceCommitEngine.audit_chain: the resident
fixed-base tables and the row MSM, rows = blocks) and the host one (CommitKey.commit + g1_sum_marshaled).  The audit
never changes the chain.  Entry 0 of the result (the genesis block, which has no step) is EMPTY.
"""
from __future__ import annotations

import dataclasses
import enum

import numpy as np

from ..native import rt


class Status(enum.IntEnum):
    OK = 0
    EMPTY = 1
    NO_COMMITMENTS = 2
    EMPTY_CHANGED = 3
    MISMATCH = 4
    BAD_POINT = 5
    INEXACT = 6
    RANGE = 7


FAILING = (Status.EMPTY_CHANGED, Status.MISMATCH, Status.BAD_POINT, Status.INEXACT, Status.RANGE)
TOL = 2.0 ** -10
KIND_EMPTY, KIND_SECAGG, KIND_PLAIN, KIND_NONE = 0, 1, 2, 3      # runtime/ledger.hpp AuditArrays::Kind
FLAG_ACCEPTED, FLAG_LEN_OK, FLAG_VEC_OK = 1, 2, 4                # AuditArrays::Flag
PASS_BLOCKS = 128   # blocks whose arrays are on the host at once (a plain block holds n x d doubles)


def w_max(scale: float) -> float:
    """The RANGE bound on |W| (see the module docstring)."""
    return 2.0 ** 40 / scale


@dataclasses.dataclass
class ChainAudit:
    status: np.ndarray      # int32 [len(chain)], Status per block
    first: np.ndarray       # int32 [len(chain)], the first offending update of the block or -1
    hash_ok: bool           # Blockchain.verify()
    hash_why: str
    backend: str            # "device" or "host"

    @property
    def counts(self) -> dict:
        return {s.name: int((self.status == int(s)).sum()) for s in Status if (self.status == int(s)).any()}

    @property
    def first_failing(self):
        bad = np.flatnonzero(np.isin(self.status, [int(s) for s in FAILING]))
        return int(bad[0]) if bad.size else None

    @property
    def ok(self) -> bool:
        return bool(self.hash_ok) and self.first_failing is None

    def lines(self) -> list:
        """One line per block that is not OK or EMPTY."""
        out = []
        for b in np.flatnonzero((self.status != Status.OK) & (self.status != Status.EMPTY)):
            s = f"block {int(b)} (iteration {int(b) - 1}): {Status(int(self.status[b])).name}"
            if self.first[b] >= 0:
                s += f" at update {int(self.first[b])}"
            out.append(s)
        return out

    def summary(self) -> str:
        c = ", ".join(f"{k} {v}" for k, v in self.counts.items())
        ff = self.first_failing
        return (f"chain audit ({self.backend}): {len(self.status)} blocks: {c}; hashes "
                f"{'ok' if self.hash_ok else 'FAILED (' + self.hash_why + ')'}; "
                + ("no failing block" if ff is None else f"first failing block {ff}"))


def _initial(a: dict):
    """The statuses before either backend runs: final for blocks with nothing to compute; plain blocks are decided
    from their rows afterwards (NO_COMMITMENTS keeps the block-level check off them)."""
    kind, flags = a["kind"], a["flags"]
    status = np.select([kind == KIND_EMPTY, kind == KIND_SECAGG], [Status.EMPTY, Status.OK],
                       Status.NO_COMMITMENTS).astype(np.int32)
    pf = flags[a["plain_update"]]
    pstatus = np.where((pf & FLAG_LEN_OK) == 0, Status.BAD_POINT,
                       np.where((pf & FLAG_VEC_OK) == 0, Status.MISMATCH, Status.OK)).astype(np.int32)
    return status, pstatus


def _host_backend(a: dict, key, scale: float, status: np.ndarray, pstatus: np.ndarray):
    R = rt()
    models, kind, off, commits = a["models"], a["kind"], a["offsets"], a["commits"]
    valid = (R.g1_marshaled_valid(commits) != 0) & ((a["flags"] & FLAG_LEN_OK) != 0) if len(commits) else \
        np.zeros((0,), bool)
    first = np.full(status.shape, -1, np.int32)
    pfirst = np.full(pstatus.shape, -1, np.int32)
    wm = w_max(scale)

    def matches(c: np.ndarray, lo: int, hi: int) -> bool:
        want = R.g1_sum_marshaled(np.ascontiguousarray(commits[lo:hi, None, :]))[0].tobytes()
        return key.commit(np.ascontiguousarray(c), 0) == want

    for k in range(len(kind)):
        w0, w1 = models[k], models[k + 1]
        if kind[k] == KIND_EMPTY:
            if not np.array_equal(w0.view(np.int64), w1.view(np.int64)):
                status[k] = Status.EMPTY_CHANGED
        elif kind[k] == KIND_SECAGG:
            with np.errstate(invalid="ignore", over="ignore"):
                if not (np.abs(w0) <= wm).all() or not (np.abs(w1) <= wm).all():
                    status[k] = Status.RANGE
                    continue
                y = (w1 - w0) * scale
                ry = np.rint(y)
                if (np.abs(y - ry) > TOL).any():
                    status[k] = Status.INEXACT
                    continue
            lo, hi = int(off[k]), int(off[k + 1])
            bad = np.flatnonzero(~valid[lo:hi])
            if bad.size:
                status[k], first[k] = Status.BAD_POINT, bad[0]
            elif not matches(ry.astype(np.int64), lo, hi):
                status[k] = Status.MISMATCH
    for r, u in enumerate(a["plain_update"]):
        if pstatus[r] != Status.OK:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            y = a["plain_delta"][r] * scale
            if not (np.abs(y) < 2.0 ** 62).all():
                pstatus[r] = Status.RANGE
                continue
        if not valid[u]:
            pstatus[r], pfirst[r] = Status.BAD_POINT, 0
        elif not matches(y.astype(np.int64), int(u), int(u) + 1):
            pstatus[r] = Status.MISMATCH
    return status, first, pstatus, pfirst


def _device_backend(a: dict, engine, scale: float, status: np.ndarray, pstatus: np.ndarray, slab):
    L, npl = status.size, pstatus.size
    res = np.concatenate([status, np.full(L, -1, np.int32), pstatus, np.full(npl, -1, np.int32)]).astype(np.int32)
    len_ok = ((a["flags"] & FLAG_LEN_OK) != 0).astype(np.int32)
    res = engine.audit_chain(a["models"], a["kind"], a["offsets"], a["commits"], len_ok, a["plain_delta"],
                             a["plain_update"], res, scale, TOL, w_max(scale), slab)
    return res[:L], res[L:2 * L], res[2 * L:2 * L + npl], res[2 * L + npl:]


def _plain_blocks(a: dict, status, first, pstatus) -> None:
    """A plain block's verdict from its rows, then its model step against the accepted deltas' sum."""
    kind, off, flags, models = a["kind"], a["offsets"], a["flags"], a["models"]
    row_of = {int(u): r for r, u in enumerate(a["plain_update"])}
    for k in np.flatnonzero(kind == KIND_PLAIN):
        lo, hi = int(off[k]), int(off[k + 1])
        rows = [row_of[u] for u in range(lo, hi)]
        st = pstatus[rows]
        bad = np.flatnonzero(st != Status.OK)
        if bad.size:
            status[k], first[k] = st[bad[0]], bad[0]
            continue
        w0, w1 = models[k], models[k + 1]
        acc = [r for r, u in zip(rows, range(lo, hi)) if flags[u] & FLAG_ACCEPTED]
        dv = a["plain_delta"][acc]
        if not (np.isfinite(w0).all() and np.isfinite(w1).all() and np.isfinite(dv).all()):
            status[k] = Status.RANGE
            continue
        total, mag = w0.copy(), np.abs(w0)
        for v in dv:
            total += v
            mag += np.abs(v)
        bound = (len(acc) + 2) * 2.0 ** -52 * mag
        status[k] = Status.OK if (np.abs(w1 - total) <= bound).all() else Status.MISMATCH


def audit_chain(chain, commit_key=None, precision: int = 4, device=None, engine=None, slab=None) -> ChainAudit:
    """Audit every block of `chain` (runtime Blockchain) under `commit_key` (runtime CommitKey).

    device: "cpu" for the host backend; None picks the GPU when there is one.  engine: a resident
    ops.bn256.DeviceCommitEngine to reuse (a running BiscottiEngine passes its own, so no second set of tables
    is built; commit_key may then be None).  slab: rows per pass of the device backend (default
    DeviceCommitEngine.AUDIT_SLAB)."""
    use_gpu = engine is not None
    if not use_gpu and str(device or "") != "cpu":
        import torch

        use_gpu = torch.cuda.is_available()
        if not use_gpu and device is not None:
            raise RuntimeError(f"chain audit on {device}: no GPU available")
    if commit_key is None and engine is None:
        raise ValueError("audit_chain needs the commitment key (or a device engine built from it)")
    d = engine.d if engine is not None else len(commit_key)
    if use_gpu and engine is None:
        from ..ops.bn256 import DeviceCommitEngine

        engine = DeviceCommitEngine(commit_key, 10, 21, device or "cuda")
    scale = 10.0 ** precision
    n = len(chain)
    status = np.full(n, Status.EMPTY, np.int32)
    first = np.full(n, -1, np.int32)
    for b0 in range(1, n, PASS_BLOCKS):
        b1 = min(n, b0 + PASS_BLOCKS)
        a = chain.audit_arrays(d, b0, b1)
        st, pst = _initial(a)
        if use_gpu:
            st, fi, pst, _ = _device_backend(a, engine, scale, st, pst, slab)
        else:
            st, fi, pst, _ = _host_backend(a, commit_key, scale, st, pst)
        st, fi = st.copy(), fi.copy()
        _plain_blocks(a, st, fi, pst)
        status[b0:b1], first[b0:b1] = st, fi
    hash_ok, why = chain.verify()
    return ChainAudit(status, first, bool(hash_ok), why, "device" if use_gpu else "host")
