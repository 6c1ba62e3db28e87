"""Batched verifySecret audit of every committed aggregate (K13; kyber.go:650-673, defined but never
called on the reference's path).

verifySecret is linear in (C, W, y), so each rank checks its own partial aggregate: a random linear
combination over every (chunk, share point) of KZG_BATCH_ROUNDS rounds (device sums, kzg.hip) and
ONE host three-pairing product per batch (pairing.cpp, prepared G2 lines).  Only aggregates that end
in the chain are audited (staged when the block is adopted, not when the aggregate is queued), and a
failed batch is re-checked round by round so failures are attributed to the right iterations.
Failures are counted and logged; they never block the chain.

--kzg-audit shares runs the consistent check per worker update instead: one row kernel over the share MSM's
output where it lies (kzg.hip k_kzg_rows; every row's triple under a seed of its own, and their sum), one pairing
product on the summed triple per block and, only if that fails, one per audited row to name the workers.
"""
from __future__ import annotations

import numpy as np
import torch

from ..utils import streams as S

KZG_BATCH_ROUNDS = 16   # rounds whose audits share one pairing product (sums of independent RLCs)


class KzgAuditMixin:
    def _kzg_init(self, cfg) -> None:
        self._kzg_pending: list = []   # launched audits (device) or checked ones (CPU)
        self._kzg_stage: list = []     # rounds waiting for the next device launch
        if cfg.kzg_audit != "off":
            self.stats.update(kzg_checks=0, kzg_failures=0)
            if cfg.kzg_audit == "shares":
                self.stats.update(kzg_share_checks=0, kzg_share_failures=0)
                self.kzg_share_blame: list = []   # (iteration, peer id) of every failing worker update
            # G2 side = (g2key[0], g2key[1]) = (G2, s G2)
            self._kzg_g2 = (self.R.g2_generator(), self._commit_key_g2_1(cfg.commit_key))
            self._kzg_rng = np.random.default_rng([cfg.seed, self.comm.rank, 0x6B7A67])

    def _commit_key_g2_1(self, path):
        """s G2 -- commitKey.json's Skey of Id 1 (publicKey.go:26-61), or 2 G2 for the generated key."""
        if path:
            import base64
            import json
            with open(path) as f:
                for ln in f:
                    if ln.strip():
                        rec = json.loads(ln)
                        if rec.get("Id") == 1:
                            return base64.b64decode(rec["Skey"])
            raise ValueError(f"{path}: no commit key record with Id 1")
        return self.R.g2_mul(self.R.g2_generator(), 2)

    # ---------------------------------------------------------------- staging (adopted aggregates only)
    def _kzg_adopt(self, agg: dict, it: int) -> None:
        """The aggregate `agg` (from _aggregate) is in the chain: stage its audit.  Device path: the
        audit stream waits for the events recorded where the sums were produced (not for work queued
        since), then the inputs join the batch."""
        rows = agg.get("kzg_rows")
        if rows is not None:   # --kzg-audit shares: launched when the aggregate was queued (GPU), or checked here
            self._kzg_pending.append(rows if self.gpu else self._kzg_host_rows(*rows, agg["xs"], it))
            return
        kin = agg.get("kzg_in")
        if kin is None:
            return
        cs_k, ws_k, y_k, xs = kin
        if not self.gpu:
            self._kzg_host(cs_k, ws_k, y_k, agg["xs"], it)
            return
        st = self.vrf_stream
        for ev in agg["kzg_events"]:
            st.wait_event(ev)
        for t in (cs_k, ws_k, y_k, xs):
            t.record_stream(st)
        with S.use(st):
            self._kzg_queue(cs_k, ws_k, y_k, xs, it)

    def _kzg_queue(self, csum, wsum, ys, xs_t, it) -> None:
        """Stage one round's aggregate for the device RLC sums (on the audit stream, current here);
        KZG_BATCH_ROUNDS rounds with the same share-point layout go into ONE launch and one pairing
        product, read back and checked later (_kzg_poll), off the round's critical path."""
        npts = ys.shape[1]
        spm = self.pc.shares_per_miner
        if self._kzg_stage and self._kzg_stage[0]["npts"] != npts:
            self._kzg_launch()
        wperm = wsum.index_select(0, self.crypto.eng.kzg_order(npts, spm))   # (chunk, point) order
        self._kzg_stage.append({"cs": csum, "ws": wperm, "ys": ys, "xs": xs_t, "npts": npts, "it": it})
        if len(self._kzg_stage) >= KZG_BATCH_ROUNDS:
            self._kzg_launch()

    def _kzg_rlc(self, st: list):
        """Queue the RLC sums of the staged rounds `st` on the audit stream: (pinned host copy, event)."""
        with S.use(self.vrf_stream):
            cat = (lambda k: torch.cat([e[k] for e in st])) if len(st) > 1 else (lambda k: st[0][k])
            npts = st[0]["npts"]
            pts = self.crypto.eng.kzg_rlc(cat("cs"), cat("ws"), cat("ys"), torch.stack([e["xs"] for e in st]),
                                          npts, self.cfg.kzg_audit == "literal",
                                          int(self._kzg_rng.integers(0, 2**63)))
            host = torch.empty((3, 24), dtype=torch.int32, pin_memory=True)
            host.copy_(pts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.vrf_stream)
        return host, ev

    def _kzg_launch(self) -> None:
        st, self._kzg_stage = self._kzg_stage, []
        if not st:
            return
        host, ev = self._kzg_rlc(st)
        # the staged inputs stay alive until the batch is decided: a failed batch is re-checked per round
        self._kzg_pending.append({"its": [e["it"] for e in st], "ev": ev, "host": host, "job": None, "stage": st})

    def _kzg_host(self, cs, ws, ys, xs, it) -> None:
        """CPU path: the same random linear combination on the host (native threads), one round."""
        nch, npts = ys.shape
        spm = self.pc.shares_per_miner
        C = [bytes(c) for c in cs.numpy()]
        Wm = [bytes(w) for w in ws.numpy()]
        W = [Wm[(j // spm) * nch * spm + k * spm + j % spm] for k in range(nch) for j in range(npts)]
        bases = [self.R.g1_generator()] if self.cfg.kzg_audit == "literal" else \
            [self.crypto.key.point(self.cfg.poly_size * k) for k in range(nch)]
        pts = self.R.kzg_rlc_host(C, W, ys.numpy().reshape(-1), list(xs), bases,
                                  int(self._kzg_rng.integers(0, 2**63)), self.cfg.host_threads)
        self._kzg_pending.append({"its": [it], "ok": self.R.kzg_check(*pts, *self._kzg_g2)})

    # ---------------------------------------------------------------- per worker (--kzg-audit shares)
    def _kzg_rows_launch(self, pts, ys, alive, cols, xs, rows, it) -> dict:
        """Queue the row sums of one aggregation on the current (audit) stream and their read-back: pts / ys the share
        MSM's output rows in place, alive their flags (a copy), cols / xs the layout's contributing share slots, rows
        the worker id of each row.  Returns the pending entry (_kzg_poll decides it once the block is adopted)."""
        n = pts.shape[0]
        out = self.crypto.eng.kzg_rlc_rows(pts, ys, cols, xs, alive=alive, seed=int(self._kzg_rng.integers(0, 2**63)))
        host = torch.empty((n + 1, 3, 24), dtype=torch.int32, pin_memory=True)
        flags = torch.empty((n,), dtype=torch.int32, pin_memory=True)
        host.copy_(out, non_blocking=True)
        flags.copy_(alive, non_blocking=True)
        return {"its": [it], "ev": S.record(), "host": host, "flags": flags, "rows": list(rows), "job": None}

    def _kzg_host_rows(self, flat, ys, rows_l, peers, ccols, ycols_t, xs, it) -> dict:
        """CPU path: each kept row's RLC and pairing product on the host (native threads), under the seeds the
        device uses."""
        from ..ops.bn256 import kzg_row_seed

        nch, T = self.nchunks, self.T
        cc, yc = ccols.numpy(), ycols_t.numpy()
        bases = [self.crypto.key.point(self.cfg.poly_size * k) for k in range(nch)]
        seed = int(self._kzg_rng.integers(0, 2**63))
        bad = []
        for i, (r, w) in enumerate(zip(rows_l, peers)):
            row = flat[r].numpy()
            C = [bytes(row[c]) for c in cc]
            W = [bytes(row[k * (T + 1) + j]) for k in range(nch) for j in yc]
            y = ys[r].numpy()[:, yc].reshape(-1)
            tri = self.R.kzg_rlc_host(C, W, y, list(xs), bases, kzg_row_seed(seed, i), self.cfg.host_threads)
            if not self.R.kzg_check(*tri, *self._kzg_g2):
                bad.append(w)
        return {"its": [it], "rows_done": (len(rows_l), bad)}

    def _kzg_rows_step(self, e: dict, must: bool) -> bool:
        """Advance one per-worker entry: the pairing product of the summed triple once the sums are back, the rows'
        own products if it fails; True once it is decided and counted."""
        if "rows_done" not in e:
            n = len(e["rows"])
            if e["job"] is None and (must or e["ev"].query()):
                e["ev"].synchronize()
                e["job"] = self.R.kzg_check_device_async(e["host"][n].numpy().view(np.uint32), *self._kzg_g2)
            if not must or e["job"] is None:
                return False   # (joined only when it must be: the products run on native threads meanwhile)
            if e["job"].result():
                e["rows_done"] = (int(e["flags"].sum()), [])
            else:   # name the culprits: one product per audited row
                jobs = [(w, self.R.kzg_check_device_async(e["host"][i].numpy().view(np.uint32), *self._kzg_g2))
                        for i, w in enumerate(e["rows"]) if e["flags"][i]]
                e["rows_done"] = (len(jobs), [w for w, j in jobs if not j.result()])
        n, bad = e["rows_done"]
        it = e["its"][0]
        self.stats["kzg_checks"] += 1
        self.stats["kzg_share_checks"] += n
        if bad:
            self.stats["kzg_failures"] += 1
            self.stats["kzg_share_failures"] += len(bad)
            self.kzg_share_blame += [(it, w) for w in bad]
            self.log.info("KZG audit (verifySecret per worker) failed in iteration %d for the updates of peers %s",
                          it, bad)
        return True

    def _kzg_share_summary(self) -> None:
        """The run's per-worker counts, logged once per change (drain)."""
        st = self.stats
        now = (st["kzg_checks"], st["kzg_share_checks"], st["kzg_share_failures"])
        if now != getattr(self, "_kzg_share_logged", None):
            self._kzg_share_logged = now
            self.log.info("KZG audit (verifySecret per worker): %d blocks, %d worker updates checked, %d failed", *now)

    def _kzg_recheck(self, e: dict) -> list:
        """A batch of several rounds failed: check each staged round on its own (device sums +
        pairing, waited for here) and return the iterations that fail individually."""
        bad = []
        for s in e["stage"]:
            host, ev = self._kzg_rlc([s])
            ev.synchronize()
            if not self.R.kzg_check_device_async(host.numpy().view(np.uint32), *self._kzg_g2).result():
                bad.append(s["it"])
        return bad

    def _kzg_poll(self, final: bool = False) -> None:
        """Start the pairing products of launches whose sums are back, and collect finished ones (all
        of them when final, the oldest when more than two are outstanding)."""
        if final and self._kzg_stage:
            self._kzg_launch()
        keep = []
        for i, e in enumerate(self._kzg_pending):
            must = final or len(self._kzg_pending) - i > 2
            if "rows" in e or "rows_done" in e:
                if not self._kzg_rows_step(e, must):
                    keep.append(e)
                continue
            if "ok" not in e and e["job"] is None and (must or e["ev"].query()):
                e["ev"].synchronize()
                e["job"] = self.R.kzg_check_device_async(e["host"].numpy().view(np.uint32), *self._kzg_g2)
            if "ok" not in e and e["job"] is not None and must:
                e["ok"] = e["job"].result()
            if "ok" in e:
                self.stats["kzg_checks"] += len(e["its"])
                if not e["ok"]:
                    bad = self._kzg_recheck(e) if len(e.get("stage") or ()) > 1 else e["its"]
                    self.stats["kzg_failures"] += len(bad)
                    if bad:
                        self.log.info("KZG audit (verifySecret, %s) failed for the aggregates of iterations %s",
                                      self.cfg.kzg_audit, bad)
            else:
                keep.append(e)
        self._kzg_pending = keep
