"""Device ECVRF prover and verifier (kernels/vrf.hip): RFC 9381 ECVRF-EDWARDS25519-SHA512-TAI on gfx950.

The protocol computes two VRF proofs per peer per round that the reference never reads (the roles proof of
getVRFRoles, quirk Q7, and the proof half of every worker's noiser VRF, vrf.go:54-100 -- only the
64-byte output feeds the lottery).  By default nothing reads them here either; with the opt-in audit
(RunConfig.vrf_audit, `DeviceVrfProver.audit`) every batch the prover launches is verified in place by
k_vrf_verify on the same stream, right behind the prove launch: no proof travels to the host, one device
counter holds the failures.  `verify` is the stand-alone batched verifier over keys, messages and proofs
given by the caller.  Round 1 spent ~37 ms of host CPU per round on them; here the
host computes the outputs the lottery needs (VrfJob outputs_only) and the proofs are queued for the
device, batch_rounds rounds per launch on a low-priority stream; the kernel splits each proof over the
three waves of a workgroup, so a launch's latency is about one variable-base scalar multiplication.  Bit-exact with runtime/vrf.cpp
(tests/test_gpu_vrf.py), which is itself pinned to the RFC's example vector.
"""
from __future__ import annotations

import numpy as np
import torch

from ..native import hip, rt
from ..utils import h2d
from ..utils import streams as S

_TORCH_OF = {np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


def _i32(b: bytes) -> np.ndarray:
    return np.frombuffer(b, np.uint8).view(np.int32)


class DeviceVrfProver:
    ALPHA_LEN = 32

    def __init__(self, device, batch_rounds: int = 1):
        self.device = torch.device(device)
        self.btab = torch.from_numpy(_i32(rt().vrf_base_table()).copy()).to(self.device)   # [512 * 32]
        self.batch_rounds = max(1, int(batch_rounds))
        self._bufs: dict = {}
        self._row: dict[bytes, int] = {}
        self._keys: list[np.ndarray] = []
        self._keys_dev = None
        self._queue: list[tuple[list[int], bytes]] = []
        self._inflight: list = []
        self.proofs = 0
        # the audit: every flushed batch is verified in place (_verify_in_place)
        self.audit = False
        self.audit_checked = 0
        self.audit_tamper = None     # test seam: called as audit_tamper(pi, tags) on a batch's proof tensor,
        #                              on the prover's stream between its prove and its verify launch
        self._audit_fail = None      # device int32 [1]: proofs whose status is not 0
        self._audit_batches: list = []   # (tags, sizes, status int32 [n]) of the batches audited since the last
        #                                  audit_result(), kept only to locate the first failure: dropped there,
        #                                  and no longer kept once it is known
        self._audit_first = None     # the run's first failure (audit_result)
        self._vbufs: dict = {}       # stream -> verifier scratch (the tables of H, Gamma and Y per proof)

    def _rows(self, seeds) -> list[int]:
        out = []
        for s in seeds:
            r = self._row.get(s)
            if r is None:
                r = self._row[s] = len(self._keys)
                self._keys.append(_i32(rt().vrf_key_material(s)))
                self._keys_dev = None
            out.append(r)
        return out

    def prove(self, seeds, alphas, beta: bool = False):
        """Proofs of seeds[i] over alphas[i] (32-byte messages) on the current stream: (pi uint8
        [n, 80], beta uint8 [n, 64] or None).  Asynchronous: read the tensors after a sync."""
        assert len(alphas) == len(seeds) and all(len(a) == self.ALPHA_LEN for a in alphas)
        uniq = {a: i for i, a in enumerate(dict.fromkeys(alphas))}
        return self._launch(np.asarray(self._rows(seeds), np.int32), list(uniq),
                            np.asarray([uniq[a] for a in alphas], np.int32), beta)

    def _launch(self, rows: np.ndarray, alphas: list, alpha_idx: np.ndarray, beta: bool = False, reuse: bool = False,
                urgent: bool = False):
        n = int(rows.size)
        if self._keys_dev is None:
            self._keys_dev = self._upload(np.concatenate(self._keys))
        al = self._upload(np.frombuffer(b"".join(alphas), np.uint8))
        idx = self._upload(np.concatenate([rows, alpha_idx]))
        # scratch and the (discarded) proofs reuse one buffer per stream: launches on a stream run in order,
        # and a fresh multi-MB allocation inside a timed round could cost a hipMalloc
        key = S.raw()
        buf = self._bufs.get(key) if reuse else None
        if not reuse:
            buf = (torch.empty((max(n, 1), 320), dtype=torch.int32, device=self.device),
                   torch.empty((max(n, 1), 80), dtype=torch.uint8, device=self.device))
        elif buf is None or buf[0].shape[0] < max(n, 1):
            cap = max(n, 1, self.batch_rounds * 256)
            buf = self._bufs[key] = (torch.empty((cap, 320), dtype=torch.int32, device=self.device),
                                     torch.empty((cap, 80), dtype=torch.uint8, device=self.device))
        scratch, pi = buf[0][: max(n, 1)], buf[1][:n]
        bt = torch.empty((n, 64), dtype=torch.uint8, device=self.device) if beta else None
        err = hip().bsc_vrf_prove_p(self._keys_dev.data_ptr(), idx.data_ptr(), al.data_ptr(), idx[n:].data_ptr(),
                                    self.ALPHA_LEN, n, self.btab.data_ptr(), scratch.data_ptr(), pi.data_ptr(),
                                    bt.data_ptr() if bt is not None else None, int(urgent), S.raw())
        if err != 0:
            raise RuntimeError(f"HIP launch of vrf_prove failed with hipError {err}")
        self.proofs += n
        self._last_uploads = (idx, al) if self.audit else None
        return pi, bt

    def reserve(self, stream, n: int) -> None:
        """Allocate the batched launches' scratch / proof buffers for n proofs now (engine warm-up), not at
        the first flush inside the timed rounds."""
        with S.use(stream):
            key = S.raw()
            cap = max(n, 1, self.batch_rounds * 256)
            buf = self._bufs.get(key)
            if buf is None or buf[0].shape[0] < cap:
                self._bufs[key] = (torch.empty((cap, 320), dtype=torch.int32, device=self.device),
                                   torch.empty((cap, 80), dtype=torch.uint8, device=self.device))
            if self.audit:
                self._verify_scratch(cap)
                if self._audit_fail is None:
                    self._audit_fail = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _upload(self, a: np.ndarray) -> torch.Tensor:
        # through the pinned staging ring (utils.h2d), stream-ordered: a pageable .to(device) blocks
        # behind the round's queued kernels, and a fresh pin_memory() costs ~1 ms of host time
        return h2d(np.ascontiguousarray(a), _TORCH_OF[a.dtype], self.device)

    # ---- round-batched queue: the engine submits each round's proofs, one launch per batch_rounds
    def submit(self, seeds, alpha: bytes, stream, expect: bytes | None = None, tag=None) -> None:
        """seeds: the proving keys' seeds, or already their key rows (int32 array, _rows).  The audit only:
        expect -- the expected 64-byte outputs of the round's first len(expect) // 64 proofs; tag -- what the
        caller wants back with the round's statuses (audit_result)."""
        if len(seeds):
            # key rows resolved now, so a flush only concatenates
            rows = seeds if isinstance(seeds, np.ndarray) else np.asarray(self._rows(seeds), np.int32)
            assert expect is None or (len(expect) % 64 == 0 and len(expect) // 64 <= rows.size)
            self._queue.append((rows, bytes(alpha), expect, tag))
        if len(self._queue) >= self.batch_rounds:
            self.flush(stream)

    def flush(self, stream, urgent: bool = False) -> None:
        """Launch the queued rounds' proofs.  urgent: the caller's next step waits for them (the run's final
        flush) -- they run at the highest wave priority instead of filling the round's idle issue slots."""
        if not self._queue:
            return
        q, self._queue = self._queue, []
        if len(q) == 1:
            # one round (one message): rows, zero message indices and the 32-byte message in ONE upload
            rows, alpha = q[0][:2]
            n = int(rows.size)
            buf = np.zeros(2 * n + len(alpha) // 4, np.int32)
            buf[:n] = rows
            buf[2 * n:] = np.frombuffer(alpha, np.int32)
            with S.use(stream):
                if self._keys_dev is None:
                    self._keys_dev = self._upload(np.concatenate(self._keys))
                up = self._upload(buf)
                scratch = torch.empty((n, 320), dtype=torch.int32, device=self.device)
                pi = torch.empty((n, 80), dtype=torch.uint8, device=self.device)
                err = hip().bsc_vrf_prove_p(self._keys_dev.data_ptr(), up.data_ptr(), up[2 * n:].data_ptr(),
                                            up[n:].data_ptr(), self.ALPHA_LEN, n, self.btab.data_ptr(),
                                            scratch.data_ptr(), pi.data_ptr(), None, int(urgent), S.raw())
                if err != 0:
                    raise RuntimeError(f"HIP launch of vrf_prove failed with hipError {err}")
                self.proofs += n
                if self.audit:
                    self._verify_in_place(up, up[2 * n:], n, pi, q, urgent)
                ev = S.record(stream)
            self._inflight.append((ev, (pi, scratch, up)))
            self._inflight = [x for x in self._inflight if not x[0].query()] if len(self._inflight) > 4 \
                else self._inflight
            return
        rows = np.concatenate([e[0] for e in q])
        alpha_idx = np.repeat(np.arange(len(q), dtype=np.int32), [e[0].size for e in q])
        with S.use(stream):   # uploads, scratch and the launch all on the prover's stream
            pi, _ = self._launch(rows, [e[1] for e in q], alpha_idx, reuse=True, urgent=urgent)
            if self.audit:
                idx, al = self._last_uploads
                self._verify_in_place(idx, al, int(rows.size), pi, q, urgent)
            ev = S.record(stream)
        self._inflight.append((ev, pi))
        # keep the last few batches alive until their kernels finished (the proofs are discarded)
        self._inflight = [x for x in self._inflight if not x[0].query()] if len(self._inflight) > 2 else self._inflight

    def drain(self, stream) -> None:
        self.flush(stream, urgent=True)
        for ev, _ in self._inflight:
            S.host_wait(ev)
        self._inflight = []

    # ---- the verifier
    def _verify_scratch(self, n: int) -> torch.Tensor:
        key = S.raw()
        buf = self._vbufs.get(key)
        if buf is None or buf.shape[0] < max(n, 1):
            buf = self._vbufs[key] = torch.empty((max(n, 1), 960), dtype=torch.int32, device=self.device)
        return buf

    def _verify_in_place(self, idx, al, n: int, pi, q: list, urgent: bool) -> None:
        """The audit of a batch the prover has just launched, on the current (the prover's) stream: the same
        proof buffer, key rows (idx[:n]), message indices (idx[n:2n]) and messages (al).  q: the batch's queue
        entries (rows, alpha, expect, tag)."""
        sizes = [int(e[0].size) for e in q]
        ex_idx = np.full(n, -1, np.int32)
        ex, off, m = [], 0, 0
        for e, k in zip(q, sizes):
            if e[2]:
                j = len(e[2]) // 64
                ex_idx[off:off + j] = np.arange(m, m + j, dtype=np.int32)
                ex.append(np.frombuffer(e[2], np.int32))
                m += j
            off += k
        eu = self._upload(np.concatenate([ex_idx] + ex)) if m else None   # indices and outputs in ONE upload
        if self._audit_fail is None:
            self._audit_fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        scratch = self._verify_scratch(n)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if self.audit_tamper is not None:
            self.audit_tamper(pi, [e[3] for e in q])
        err = hip().bsc_vrf_verify(self._keys_dev.data_ptr() + 64, 24, idx.data_ptr(), al.data_ptr(),
                                   idx[n:].data_ptr(), self.ALPHA_LEN, n, self.btab.data_ptr(), scratch.data_ptr(),
                                   pi.data_ptr(), eu[n:].data_ptr() if m else None, eu.data_ptr() if m else None,
                                   status.data_ptr(), None, self._audit_fail.data_ptr(), int(urgent), S.raw())
        if err != 0:
            raise RuntimeError(f"HIP launch of vrf_verify failed with hipError {err}")
        self.audit_checked += n
        if self._audit_first is None:
            self._audit_batches.append(([e[3] for e in q], sizes, status))

    def audit_result(self):
        """After drain: (proofs checked, failures, first failure or None).  The first failure is (tag of its
        round, index of the proof in the round, status); the statuses are read only while the counter is not
        zero and the first failure not known yet.  The batches' statuses are dropped here."""
        fails = int(self._audit_fail.item()) if self._audit_fail is not None else 0
        if fails and self._audit_first is None:
            for tags, sizes, status in self._audit_batches:
                st = status.cpu().numpy()
                bad = np.flatnonzero(st)
                if bad.size:
                    i, off = int(bad[0]), 0
                    for tag, k in zip(tags, sizes):
                        if i < off + k:
                            self._audit_first = (tag, i - off, int(st[i]))
                            break
                        off += k
                    break
        self._audit_batches = []
        return self.audit_checked, fails, self._audit_first

    def verify(self, pks, alphas, pis, expect=None):
        """Batched verification on the current stream of pis[i] (80 bytes) as the proof of the key pks[i]
        (32 bytes, encoded) over alphas[i] (messages of one length, at most 1024 bytes): (status int32 [n],
        beta uint8 [n, 64]).  Status 0: valid, beta is the output; 1 / 2: the key / Gamma does not decode;
        3: s >= L; 4: the challenge differs; 5: valid, but the output differs from expect[i] (64 bytes, or None
        for no expectation).  beta is zero for status 1..4.  Asynchronous: read the tensors after a sync."""
        n = len(pis)
        if not (len(pks) == n and len(alphas) == n):
            raise ValueError("verify: pks, alphas and pis differ in length")
        alen = len(alphas[0]) if n else 0
        if alen > 1024 or any(len(a) != alen for a in alphas):
            raise ValueError("verify: the messages must have one length of at most 1024 bytes")
        if any(len(k) != 32 for k in pks) or any(len(p) != 80 for p in pis):
            raise ValueError("verify: a key is 32 bytes, a proof 80")
        if expect is not None and (len(expect) != n or any(e is not None and len(e) != 64 for e in expect)):
            raise ValueError("verify: expect holds one 64-byte output (or None) per proof")
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        beta = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        if n == 0:
            return status, beta
        uk = {k: i for i, k in enumerate(dict.fromkeys(pks))}
        ua = {a: i for i, a in enumerate(dict.fromkeys(alphas))}
        keys = self._upload(np.frombuffer(b"".join(uk), np.uint8).view(np.int32))
        al = self._upload(np.frombuffer(b"".join(ua) + bytes(4), np.uint8))
        idx = self._upload(np.asarray([uk[k] for k in pks] + [ua[a] for a in alphas], np.int32))
        pi = self._upload(np.frombuffer(b"".join(pis), np.uint8))
        eu, m = None, 0
        if expect is not None and any(e is not None for e in expect):
            have = [e for e in expect if e is not None]
            m = len(have)
            it = iter(range(m))
            ex_idx = np.asarray([next(it) if e is not None else -1 for e in expect], np.int32)
            eu = self._upload(np.concatenate([ex_idx, np.frombuffer(b"".join(have), np.int32)]))
        scratch = torch.empty((n, 960), dtype=torch.int32, device=self.device)
        err = hip().bsc_vrf_verify(keys.data_ptr(), 8, idx.data_ptr(), al.data_ptr(), idx[n:].data_ptr(), alen, n,
                                   self.btab.data_ptr(), scratch.data_ptr(), pi.data_ptr(),
                                   eu[n:].data_ptr() if m else None, eu.data_ptr() if m else None,
                                   status.data_ptr(), beta.data_ptr(), None, 0, S.raw())
        if err != 0:
            raise RuntimeError(f"HIP launch of vrf_verify failed with hipError {err}")
        return status, beta
