"""The device Schnorr verifier of the engine and the opt-in audit of the signatures a rank's own verifiers produce
(RunConfig.sig_audit, --sig-audit; not in the reference).

The audit and the miners' quorum check (--verify-signatures, Q5: secagg.py _sig_filter) go through one
`ops.schnorr.SchnorrVerifier` (kernels/schnorr.hip, k_schnorr_verify), created lazily at the first use (_sig_verifier)
-- with neither flag set no table is built and no launch is added -- and again when a peer's key has changed.

The audit (_sig_audit_batch): where _join_signatures (verify.py) receives a batch, item (v, j) is sig_np[v, j] over
the commitment of worker inboxes[v][j] under pk[v], accepted slots only; commitment and key are taken where the batch
is signed.  On a GPU one launch on a low-priority side stream into a device counter; nothing is read before drain()
(a run that holds more than SIG_AUDIT_KEEP batches waits for the audit stream and reads its oldest half, to bound
what it keeps; engine.sig_audit_keep overrides the bound).  On the CPU, or for status 3 (the draw cap), the host verifier
decides.  drain() sets stats["sig_audit_checked"] and stats["sig_audit_failures"] and logs the first failure once
per run with iteration, verifier and worker.  A failure never changes the chain; no collective is added.  Test seam:
engine.sig_audit_tamper(sig_np, iteration), applied to the audit's own copy of the matrix.

The device signer (engine.sign_device, `peer --device-sign`; k_schnorr_sign) lives here too: it shares the verifier's
streams and, where the run has a verifier, its table of G.  With the switch off nothing of it is built or launched.
"""
from __future__ import annotations

import numpy as np
import torch

from ..utils import streams as S

SIG_AUDIT_KEEP = 256   # batches kept unread at most


class _DeviceSignJob:
    """What _join_signatures reads of a device batch: the host SignJob's result_array()."""

    def __init__(self, wait, stats: dict):
        self._wait, self._stats = wait, stats

    def done(self) -> bool:
        return bool(self._wait.ready())

    def result_array(self) -> np.ndarray:
        sigs, status, replaced = self._wait()
        if status.any():   # (the engine's indices are in range by construction: status 4 is a bug)
            raise RuntimeError(f"device signer: statuses {sorted(set(status[status != 0].tolist()))} left unsigned")
        self._stats["sign_device"] = self._stats.get("sign_device", 0) + int(status.size) - replaced
        self._stats["sign_device_host"] = self._stats.get("sign_device_host", 0) + replaced
        return sigs


class SigAuditMixin:
    _sign_on = False                    # engine.sign_device
    _sign_dev = None                    # ops.schnorr.SchnorrSigner, lazily

    def _sig_audit_init(self, cfg) -> None:
        self._sig_dev = None            # ops.schnorr.SchnorrVerifier, lazily
        self._sig_stream = None         # the quorum check's stream (high priority: the round waits for it)
        self._sig_audit_stream = None   # the audit's (low priority: nothing waits for it before drain)
        self._sig_audit_fail = None     # device int32 [1]: items whose status is not 0
        self._sig_audit_batches: list = []   # (iteration, items [(verifier, worker)], msgs, sigs, keys, status dev, n)
        self._sig_audit_acc = {"checked": 0, "failures": 0, "first": None}
        self._sig_audit_logged = False
        if cfg.sig_audit:
            self.stats["sig_audit_checked"] = self.stats["sig_audit_failures"] = 0

    # ------------------------------------------------------------------ the shared device verifier
    def _sig_verifier(self):
        pks = [self.pk[i] for i in range(self.N)]
        sv = self._sig_dev
        if sv is None or sv.pks != pks:   # the first use, or a restart has changed a key
            from ..ops.schnorr import SchnorrVerifier

            if sv is not None:
                torch.cuda.synchronize(self.dev)
                sv.release()
            self._sig_streams()
            with S.use(self._sig_stream):
                sv = self._sig_dev = SchnorrVerifier(pks, self.dev)
            torch.cuda.synchronize(self.dev)   # the tables are visible to every stream
            self.stats["sig_table_bytes"] = sv.table_bytes()
        return sv

    def _sig_release(self) -> None:
        sv, self._sig_dev = self._sig_dev, None
        if sv is not None:
            sv.release()
        sg, self._sign_dev = self._sign_dev, None
        if sg is not None:
            sg.release()
        self._sig_stream = self._sig_audit_stream = None

    # ------------------------------------------------------------------ engine.sign_device (--device-sign)
    @property
    def sign_device(self) -> bool:
        """The verifiers' signatures come from k_schnorr_sign (ops.schnorr.SchnorrSigner) instead of the host's
        SignJob: the same bytes.  Off by default; on a CPU engine the switch is accepted and the host signs.
        Stats (present once the switch has been set): sign_device (signatures the kernel produced),
        sign_device_host (status-3 items the host signed), sign_table_bytes (0 for a borrowed table)."""
        return self._sign_on

    @sign_device.setter
    def sign_device(self, on) -> None:
        self._sign_on = bool(on)
        if self._sign_on:
            for k in ("sign_device", "sign_device_host", "sign_table_bytes"):
                self.stats.setdefault(k, 0)

    def _sig_streams(self) -> None:
        if self._sig_stream is None:
            lo, hi = torch.cuda.Stream.priority_range()
            self._sig_stream = torch.cuda.Stream(device=self.dev, priority=hi)
            self._sig_audit_stream = torch.cuda.Stream(device=self.dev, priority=lo)

    def _sig_signer(self):
        """The engine's device signer, created at the first signed batch; it borrows the verifier's table of G
        where this run has a verifier (--verify-signatures, --sig-audit)."""
        sg = self._sign_dev
        if sg is None:
            from ..ops.schnorr import SchnorrSigner

            cfg = self.cfg
            wanted = cfg.sig_audit or (cfg.verify_signatures and cfg.verification and cfg.secure_agg)
            sv = self._sig_verifier() if (self._sig_dev is not None or wanted) else None
            self._sig_streams()
            with S.use(self._sig_stream):
                sg = self._sign_dev = SchnorrSigner(self.dev, table=sv)
            torch.cuda.synchronize(self.dev)   # the table is visible to every stream
            self.stats["sign_table_bytes"] = sg.table_bytes()
        return sg

    def _sign_on_device(self, msgs: np.ndarray, msg_idx, key_of, nonce_ids, sks: list, bases: list, waited: bool):
        """Launch one batch of verifier signatures (verify.py _prep_sign) and return its job: result_array() waits
        for the read-back and lets the host sign what the kernel left undecided.  waited: the round reads this
        batch before its block (the high-priority stream); a deferred batch goes on the low-priority one."""
        sg = self._sig_signer()
        with S.use(self._sig_stream if waited else self._sig_audit_stream):
            wait = sg.sign_resolved(msgs, msg_idx, key_of, nonce_ids, sks, bases)
        return _DeviceSignJob(wait, self.stats)

    # ------------------------------------------------------------------ --sig-audit
    def _sig_audit_host(self, it: int, items: list, msgs, pks: list, sigs, which) -> None:
        """The host verifier's verdict on items `which` (indices)."""
        acc = self._sig_audit_acc
        for i in which:
            if not self.R.schnorr_verify(msgs[i].tobytes(), pks[i], sigs[i].tobytes()):
                acc["failures"] += 1
                if acc["first"] is None:
                    acc["first"] = (it, *items[i])

    def _sig_audit_batch(self, sig_np: np.ndarray, sl, msgs, pks, plan, inboxes: dict, it: int) -> None:
        """Audit the signatures of one joined batch: sl = (verifier index in the plan, inbox slot) of each; msgs
        (uint8 [n, 64]) the commitment each one signs and pks (64 bytes each) its verifier's public key, both as
        they stood when the batch was signed (a deferred batch is joined up to two rounds later: the pinned
        commitment rows have moved on by then, and a restart may have replaced a key)."""
        tamper = getattr(self, "sig_audit_tamper", None)
        if tamper is not None:
            sig_np = sig_np.copy()
            tamper(sig_np, it)
        if sl is None or len(sl[0]) == 0:
            return
        sl_v, sl_j = np.asarray(sl[0], np.int64), np.asarray(sl[1], np.int64)
        verifiers = [plan.verifiers[int(k)] for k in sl_v]
        workers = [inboxes[v][int(j)] for v, j in zip(verifiers, sl_j)]
        sigs = np.ascontiguousarray(sig_np[sl_v, sl_j])            # [n, 64]
        msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 64)
        items = list(zip(verifiers, workers))
        n = len(items)
        assert msgs.shape[0] == n and len(pks) == n
        self._sig_audit_acc["checked"] += n
        if not self.gpu:
            self._sig_audit_host(it, items, msgs, pks, sigs, range(n))
            return
        sv = self._sig_verifier()
        # the table holds the keys as they stand now: an item signed under a key replaced since goes to the host
        stale = [i for i, v in enumerate(verifiers) if sv.pks[v] != pks[i]]
        if stale:
            self._sig_audit_host(it, items, msgs, pks, sigs, stale)
            keep = np.setdiff1d(np.arange(n), stale)
            items, pks = [items[i] for i in keep], [pks[i] for i in keep]
            msgs, sigs, verifiers = msgs[keep], sigs[keep], [verifiers[i] for i in keep]
            n = len(items)
            if n == 0:
                return
        if self._sig_audit_fail is None:
            self._sig_audit_fail = torch.zeros(1, dtype=torch.int32, device=self.dev)
            torch.cuda.current_stream(self.dev).synchronize()
        mi = np.arange(n, dtype=np.int32)
        ki = np.asarray(verifiers, np.int32)
        with S.use(self._sig_audit_stream):
            status, _ = sv.launch(msgs, mi, ki, sigs, self._sig_audit_fail)
        self._sig_audit_batches.append((it, items, msgs, pks, sigs, status, n))
        keep_max = getattr(self, "sig_audit_keep", SIG_AUDIT_KEEP)
        if len(self._sig_audit_batches) > keep_max:
            k = max(1, keep_max // 2)
            old, self._sig_audit_batches = self._sig_audit_batches[:k], self._sig_audit_batches[k:]
            self._sig_audit_collect(old)

    def _sig_audit_collect(self, batches: list) -> None:
        """Read the statuses of `batches`, once the audit stream has finished them; the host verifier decides
        status 3."""
        self._sig_audit_stream.synchronize()
        acc = self._sig_audit_acc
        for it, items, msgs, pks, sigs, status, n in batches:
            st = status[:n].cpu().numpy()
            for i in np.flatnonzero(st):
                if st[i] == 3 and self.R.schnorr_verify(msgs[i].tobytes(), pks[i], sigs[i].tobytes()):
                    continue
                acc["failures"] += 1
                if acc["first"] is None:
                    acc["first"] = (it, *items[i])

    def _sig_audit_finish(self) -> None:
        """drain(): read the device counter (the statuses only when it is not zero), set the stats, log the first
        failure once."""
        acc = self._sig_audit_acc
        batches, self._sig_audit_batches = self._sig_audit_batches, []
        if batches:
            self._sig_audit_stream.synchronize()
            if int(self._sig_audit_fail.item()):   # (batches read earlier have left their count in it too)
                self._sig_audit_collect(batches)
            self._sig_audit_fail.zero_()
        self.stats["sig_audit_checked"], self.stats["sig_audit_failures"] = acc["checked"], acc["failures"]
        if acc["failures"] and not self._sig_audit_logged:
            self._sig_audit_logged = True
            self.log.info("Signature audit: %d of %d signatures failed; the first one in iteration %d, verifier %d, "
                          "worker %d", acc["failures"], acc["checked"], *acc["first"])
