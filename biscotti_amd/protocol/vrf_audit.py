"""The opt-in audit of the round's VRF proofs (RunConfig.vrf_audit, --vrf-audit; not in the reference).

Every rank checks the proofs it produced -- each local worker's noiser proof and each live local peer's roles
proof (Q7) -- and adds no collective:

  * device batches: the prover verifies each batch in place right behind its prove launch (ops/vrf.py
    _verify_in_place, kernels/vrf.hip k_vrf_verify), on the VRF stream at the batch's priority class, into one
    device failure counter.  The noiser proofs carry the host output that fed the noiser lottery: a valid proof
    of another output is a failure too (status 5).  Roles proofs have no host output on that path.
  * host proofs (the run's last round on a GPU; every proof without a GPU or with --no-vrf-device): the host
    verifier (runtime/vrf.cpp vrf_verify) when their job is joined.

drain() sets stats["vrf_audit_checked"] and stats["vrf_audit_failures"] and logs the first failure once per
run.  Like the KZG audit, a failure never changes the chain.  The audit changes neither which batches the
prover launches nor when: it only gives submit() the expected outputs and the round's tag.

Test seam (one place): engine.vrf_dev.audit_tamper, a callable (pi, tags) the prover applies to a batch's proof
tensor (uint8 [n, 80]) on the VRF stream between its prove and its verify launch; tags: the batch's rounds as
(iteration, peers).
"""
from __future__ import annotations

import time


class VrfAuditMixin:
    def _vrf_audit_init(self, cfg) -> None:
        self._vrf_audit_jobs: list = []   # host proofs whose job is not joined yet
        self._vrf_audit_host = {"checked": 0, "failures": 0, "first": None, "join_ms": 0.0, "verify_ms": 0.0}
        self._vrf_audit_logged = False
        if cfg.vrf_audit:
            self.stats["vrf_audit_checked"] = self.stats["vrf_audit_failures"] = 0

    def _vrf_audit_expect(self, head: dict, local_workers: list) -> list:
        """The 64-byte outputs that fed _select_noisers for local_workers, in that order."""
        fut = head.get("fut_noise")
        if fut is None or not local_workers:
            return []
        betas = fut.betas()
        idx = head.get("vrf_index")
        return [betas[i] for i in idx] if idx is not None else betas[:len(local_workers)]

    def _vrf_audit_args(self, head: dict, lw: list, lv, it: int) -> dict:
        """What the audit adds to the device prover's submit() of a round's proofs: the noiser proofs' expected
        outputs (they lead the round's rows) and the round's tag (iteration, peers) for the failure log."""
        peers = list(lw) + ([p for p in self.local if lv[p]] if self.cfg.roles_vrf_proof else [])
        return {"expect": b"".join(self._vrf_audit_expect(head, lw)), "tag": (it, peers)}

    def _vrf_audit_host_job(self, job, seeds: list, index, alpha: bytes, expect, it: int, peers: list) -> None:
        """Queue a host job's proofs for the host verifier: proof index[i] (None: i) of the job belongs to
        seeds[i] / peers[i]; expect: the outputs the lottery consumed, None (as a whole or per entry) where there
        is none (the roles proofs)."""
        if job is not None and seeds:
            self._vrf_audit_jobs.append((job, list(seeds), index, bytes(alpha), expect, it, list(peers)))

    def _vrf_audit_poll(self, final: bool) -> None:
        """Verify the queued host proofs whose job has finished (every one when final)."""
        acc = self._vrf_audit_host
        t0 = time.perf_counter()
        keep, todo = [], []   # todo: (pk, alpha, pi, the job's output, the lottery's or None, iteration, peer)
        for e in self._vrf_audit_jobs:
            job, seeds, index, alpha, expect, it, peers = e
            if not (final or job.done()):
                keep.append(e)
                continue
            out = job.result()
            for i, s in enumerate(seeds):
                beta, pi = out[index[i] if index is not None else i]
                todo.append((self.R.vrf_key_material(s)[64:], alpha, pi, beta,
                             expect[i] if expect is not None else None, it, peers[i]))
        self._vrf_audit_jobs = keep
        t1 = time.perf_counter()
        if len(todo) >= 32:
            # a GPU run's last round (~200 proofs, ~0.13 ms each): the binding drops the GIL, so a few threads
            # share them instead of the round's thread verifying them one after the other
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max(1, min(8, self.cfg.host_threads))) as ex:
                got_all = list(ex.map(lambda t: self.R.vrf_verify(t[0], t[1], t[2]), todo, chunksize=1))
        else:
            got_all = [self.R.vrf_verify(t[0], t[1], t[2]) for t in todo]
        acc["join_ms"] += 1e3 * (t1 - t0)
        acc["verify_ms"] += 1e3 * (time.perf_counter() - t1)
        for (_, _, _, beta, want, it, peer), got in zip(todo, got_all):
            acc["checked"] += 1
            if got is None or got != beta or (want is not None and got != want):
                acc["failures"] += 1
                if acc["first"] is None:   # the host verifier gives no status: rejected, or another output
                    acc["first"] = (it, peer, "rejected" if got is None else "output mismatch")

    def _vrf_audit_finish(self) -> None:
        """drain(): join everything, read the device counter, set the stats, log the first failure once."""
        self._vrf_audit_poll(final=True)
        acc = self._vrf_audit_host
        checked, fails, first = acc["checked"], acc["failures"], acc["first"]
        if self.vrf_dev is not None:
            dc, df, dfirst = self.vrf_dev.audit_result()
            checked += dc
            fails += df
            if dfirst is not None:   # the device batches hold every round before the host's last one
                (it, peers), i, status = dfirst
                first = (it, peers[i], "status %d" % status)
        self.stats["vrf_audit_checked"], self.stats["vrf_audit_failures"] = checked, fails
        # where the host verifier's time went (docs/PERF.md): waiting for the proving jobs / verifying their proofs
        self.stats["vrf_audit_host_join_ms"] = round(acc["join_ms"], 3)
        self.stats["vrf_audit_host_verify_ms"] = round(acc["verify_ms"], 3)
        if fails and not self._vrf_audit_logged:
            self._vrf_audit_logged = True
            self.log.info("VRF audit: %d of %d proofs failed; the first one in iteration %d, peer %d (%s)",
                          fails, checked, *first)
