"""Batched Schnorr verification on gfx950 (kernels/schnorr.hip): the verifier signatures of a round.

A signature is ``c || r`` (two 32-byte big-endian scalars) over a 64-byte message (a marshalled G1 commitment); it
is valid under the key PK iff ``c < n``, ``r < n`` and ``c == H(marshal(r G + c PK) || message)`` -- the host's
``schnorr_verify`` (runtime/bn256.cpp), which is the specification and the oracle (tests/test_gpu_schnorr.py).

`SchnorrVerifier` owns the fixed-base tables of G and of every peer key (B0 = 8, NW = 33 windows of 128 affine
entries: 270,336 bytes per base), built once with the commitment tables' builder (bsc_fb_table).  One item is a
triple (message index, key index, signature); one launch gives one status per item:

    0 valid | 1 c >= n or r >= n | 2 the challenge differs | 3 undecided after DRAWS = 32 candidate draws
    (probability 0.439^32 ~ 3.5e-12: the host decides) | 4 message or key index out of range
"""
from __future__ import annotations

import numpy as np
import torch

from ..native import hip, rt
from ..utils import d2h_into, h2d_many
from ..utils import streams as S
from .bn256 import check_fb_entries, fb_entries

B0, NW = 8, 33
PB = fb_entries(B0, NW)  # entries per base
DRAWS = 32
_BUILD_BATCH = 32        # bases per table-build launch: 33 runs x 16 KB of scratch each
VALID, RANGE, MISMATCH, UNDECIDED, INDEX = 0, 1, 2, 3, 4


def _check(err: int, what: str) -> None:
    if err != 0:
        raise RuntimeError(f"HIP launch of {what} failed with hipError {err}")


class SchnorrVerifier:
    def __init__(self, pks, device):
        """pks: the peers' 64-byte marshalled public keys, in peer order (key index k = pks[k])."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SchnorrVerifier runs on a GPU (the host verifier is rt().schnorr_verify)")
        lib = hip()   # raises without the HIP library: no eager fall-back
        R = rt()
        self.pks = [bytes(k) for k in pks]
        if not self.pks or any(len(k) != 64 for k in self.pks):
            raise ValueError("SchnorrVerifier: at least one key, each a 64-byte marshalled G1 point")
        self.nkeys = len(self.pks)
        bases = np.concatenate([R.g1_affine_mont_u32(R.g1_generator())] +
                               [R.g1_affine_mont_u32(k) for k in self.pks]).astype(np.uint32)   # [1 + N, 16]
        nb = 1 + self.nkeys
        bases_t = torch.from_numpy(np.ascontiguousarray(bases).view(np.int32)).to(self.device)
        check_fb_entries(B0, NW)   # before the table is allocated
        self.table = torch.empty((nb, PB, 16), dtype=torch.int32, device=self.device)
        scratch = torch.empty((min(_BUILD_BATCH, nb) * PB * 32,), dtype=torch.int32, device=self.device)
        for s0 in range(0, nb, _BUILD_BATCH):
            _check(lib.bsc_fb_table(bases_t.data_ptr(), 0, s0, min(_BUILD_BATCH, nb - s0), 1, B0, NW, PB, 1, 0,
                                    self.table.data_ptr(), scratch.data_ptr(), S.raw()), "fb_table")
        torch.cuda.current_stream(self.device).synchronize()
        del scratch, bases_t
        self._bufs: list = []    # every pinned read-back buffer made (verify)
        self._free: dict = {}    # capacity -> the ones no outstanding result uses

    def table_bytes(self) -> int:
        return 0 if self.table is None else self.table.numel() * 4

    def release(self) -> None:
        """Drop the device tables; the verifier is unusable afterwards.  Waits for the device: the read-back buffers go too."""
        if self.table is not None:
            torch.cuda.synchronize(self.device)   # no launch or read-back of this verifier is in flight afterwards
        self.table = None
        self._bufs, self._free = [], {}

    # ------------------------------------------------------------------ launches
    def _upload(self, messages, msg_idx, key_idx, sigs):
        msgs = np.ascontiguousarray(messages, np.uint8).reshape(-1, 64)
        sg = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 64)
        mi = np.ascontiguousarray(msg_idx, np.int32).reshape(-1)
        ki = np.ascontiguousarray(key_idx, np.int32).reshape(-1)
        n = int(sg.shape[0])
        if not (mi.size == n and ki.size == n):
            raise ValueError("verify: msg_idx, key_idx and sigs differ in length")
        if msgs.shape[0] < 1:
            raise ValueError("verify: at least one 64-byte message")
        return msgs, mi, ki, sg, n

    def launch(self, messages, msg_idx, key_idx, sigs, counter=None):
        """Upload and launch on the current stream; nothing is read back: (status int32 [n] on the device, n).
        counter: optional device int32 [1], incremented once per item whose status is not 0."""
        if self.table is None:
            raise RuntimeError("SchnorrVerifier: released")
        return self._launch(*self._upload(messages, msg_idx, key_idx, sigs), counter)

    def _launch(self, msgs, mi, ki, sg, n, counter):
        cap = max(256, (n + 255) & ~255)
        status = torch.empty((cap,), dtype=torch.int32, device=self.device)
        if n == 0:
            return status, 0
        d_msgs, d_sg, d_mi, d_ki = h2d_many([(msgs, torch.uint8), (sg, torch.uint8), (mi, torch.int32),
                                             (ki, torch.int32)], self.device)
        _check(hip().bsc_schnorr_verify(d_msgs.data_ptr(), d_mi.data_ptr(), d_ki.data_ptr(), d_sg.data_ptr(),
                                        self.table.data_ptr(), self.nkeys, int(msgs.shape[0]), n, status.data_ptr(),
                                        counter.data_ptr() if counter is not None else None, S.raw()),
               "schnorr_verify")
        return status, n

    def _host_buffer(self, cap: int) -> torch.Tensor:
        """A pinned int32 [cap] read-back buffer that no outstanding result uses: taken from the free list, or new.
        The verifier keeps every buffer it ever made (a bare copy may still be in flight when its result is
        dropped unread: such a buffer is never reused, and never returns to an allocator before release())."""
        free = self._free.setdefault(cap, [])
        if free:
            return free.pop()
        buf = torch.empty((cap,), dtype=torch.int32, pin_memory=True)
        self._bufs.append(buf)
        return buf

    def verify(self, messages, msg_idx, key_idx, sigs, counter=None):
        """One launch and one read-back on the current stream.  messages: uint8 [nmsg, 64]; msg_idx, key_idx:
        int [n]; sigs: uint8 [n, 64].  Returns a callable giving status int32 [n] (it waits for the read-back; call
        it once).  Any number of results may be outstanding: each has a pinned buffer of its own until it is read."""
        if self.table is None:
            raise RuntimeError("SchnorrVerifier: released")
        inputs = self._upload(messages, msg_idx, key_idx, sigs)
        status, n = self._launch(*inputs, counter)
        if n == 0:
            result = lambda: np.zeros(0, np.int32)   # noqa: E731
            result.ready = lambda: True
            result.inputs = inputs[:4]
            return result
        host = self._host_buffer(int(status.shape[0]))
        d2h_into(host, status)
        ev = S.record()
        box = [host, status]   # the device statuses live until the copy has been waited for

        def result():
            S.host_wait(ev)
            if box[0] is None:
                raise RuntimeError("SchnorrVerifier: a result is read once")
            out = box[0].numpy()[:n].copy()
            self._free[int(box[0].shape[0])].append(box[0])   # the copy has landed and been taken: reusable
            box[0] = box[1] = None
            return out
        result.ready = ev.query
        result.inputs = inputs[:4]   # the host arrays as uploaded (msgs, msg_idx, key_idx, sigs)
        return result

    def verify_resolved(self, messages, msg_idx, key_idx, sigs, counter=None):
        """verify() with every status 3 replaced by the host verifier's verdict (0 or 2)."""
        wait = self.verify(messages, msg_idx, key_idx, sigs, counter)
        msgs, mi, ki, sg = wait.inputs

        def result():
            st = wait()
            for i in np.flatnonzero(st == UNDECIDED):
                ok = rt().schnorr_verify(msgs[mi[i]].tobytes(), self.pks[ki[i]], sg[i].tobytes())
                st[i] = VALID if ok else MISMATCH
            return st
        result.ready = wait.ready
        return result

    # ------------------------------------------------------------------ the test entry points
    def challenge(self, tms, messages):
        """bsc_schnorr_challenge: tms, messages uint8 [n, 64] -> (scalar uint8 [n, 32] big-endian, draws int32 [n]);
        draws 0 and a zero scalar where none of DRAWS candidates fits.  Synchronous."""
        tm = np.array(tms, np.uint8).reshape(-1, 64)
        ms = np.array(messages, np.uint8).reshape(-1, 64)
        n = tm.shape[0]
        assert ms.shape[0] == n
        d_tm = torch.from_numpy(tm).to(self.device)
        d_ms = torch.from_numpy(ms).to(self.device)
        sc = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        dr = torch.zeros((n,), dtype=torch.int32, device=self.device)
        _check(hip().bsc_schnorr_challenge(d_tm.data_ptr(), d_ms.data_ptr(), n, sc.data_ptr(), dr.data_ptr(),
                                           S.raw()), "schnorr_challenge")
        return sc.cpu().numpy(), dr.cpu().numpy()

    def point(self, rs, cs, key_idx):
        """bsc_schnorr_point: rs, cs uint8 [n, 32] big-endian scalars, key_idx int [n] -> uint8 [n, 64], the
        marshal of r G + c PK (zeros for infinity or a key index out of range).  Synchronous."""
        r = np.array(rs, np.uint8).reshape(-1, 32)
        c = np.array(cs, np.uint8).reshape(-1, 32)
        ki = np.array(key_idx, np.int32).reshape(-1)
        n = r.shape[0]
        assert c.shape[0] == n and ki.size == n
        d_r, d_c, d_k = (torch.from_numpy(a).to(self.device) for a in (r, c, ki))
        out = torch.zeros((n, 64), dtype=torch.uint8, device=self.device)
        _check(hip().bsc_schnorr_point(d_r.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), self.table.data_ptr(),
                                       self.nkeys, n, out.data_ptr(), S.raw()), "schnorr_point")
        return out.cpu().numpy()


def quorum(status, groups) -> dict:
    """Host side: status int [n] of items whose (worker, signature slot) is groups[i]; returns {worker: number
    of its signature slots with at least one valid item}, every worker of `groups` present."""
    st = np.asarray(status).reshape(-1)
    g = np.asarray(groups, np.int64).reshape(-1, 2)
    assert g.shape[0] == st.size
    out = {int(w): 0 for w in np.unique(g[:, 0])} if g.size else {}
    good = np.unique(g[st == VALID], axis=0) if st.size else np.zeros((0, 2), np.int64)
    for w in good[:, 0]:
        out[int(w)] += 1
    return out
