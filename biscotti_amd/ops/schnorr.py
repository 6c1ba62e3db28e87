"""Batched Schnorr verification and signing on gfx950 (kernels/schnorr.hip): the verifier signatures of a round.

A signature is ``c || r`` (two 32-byte big-endian scalars) over a 64-byte message (a marshalled G1 commitment); it
is valid under the key PK iff ``c < n``, ``r < n`` and ``c == H(marshal(r G + c PK) || message)`` -- the host's
``schnorr_verify`` (runtime/bn256.cpp), which is the specification and the oracle (tests/test_gpu_schnorr.py).

`SchnorrVerifier` owns the fixed-base tables of G and of every peer key (B0 = 8, NW = 33 windows of 128 affine
entries: 270,336 bytes per base), built once with the commitment tables' builder (bsc_fb_table).  One item is a
triple (message index, key index, signature); one launch gives one status per item:

    0 valid | 1 c >= n or r >= n | 2 the challenge differs | 3 undecided after DRAWS = 32 candidate draws
    (probability 0.439^32 ~ 3.5e-12: the host decides) | 4 message or key index out of range

`SchnorrSigner` is the signing half (k_schnorr_sign): a round's verifier signatures in one launch over the table of
G alone, byte-identical to the host's ``schnorr_sign`` (tests/test_gpu_schnorr_sign.py).
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


def _scalar_int(x) -> int:
    return int(x) if isinstance(x, (int, np.integer)) else int.from_bytes(bytes(x), "big")


class SchnorrSigner:
    """The verifiers' signatures of a round in one launch (k_schnorr_sign); the host signer ``rt().schnorr_sign``
    is the specification, and the device writes the same 64 bytes.  Item i signs ``messages[msg_idx[i]]`` with the
    local key ``sks[key_idx[i]]`` and the nonce entropy ``bases[key_idx[i]] || le32(nonce_ids[i])``.  Status per
    item: 0 signed | 3 a XOF found no candidate within DRAWS (zero bytes: the host signs, sign_resolved) | 4 an
    index out of range (zero bytes).  Keys and nonce bases travel with each launch (at most 64 signers)."""

    def __init__(self, device, table=None):
        """table: a SchnorrVerifier whose table is borrowed (its base 0 is G), or None: a one-base table of G is
        built (270,336 bytes)."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SchnorrSigner runs on a GPU (the host signer is rt().schnorr_sign)")
        lib = hip()   # raises without the HIP library: no eager fall-back
        self.order = int(rt().bn256_order())
        self.borrowed = table is not None
        if table is not None:
            self.table = table.table   # the tensor itself: it outlives the verifier's release()
            if self.table is None:
                raise RuntimeError("SchnorrSigner: the verifier whose table is borrowed has been released")
        else:
            R = rt()
            base = np.ascontiguousarray(R.g1_affine_mont_u32(R.g1_generator())).astype(np.uint32).reshape(1, 16)
            base_t = torch.from_numpy(base.view(np.int32)).to(self.device)
            check_fb_entries(B0, NW)   # before the table is allocated
            self.table = torch.empty((1, PB, 16), dtype=torch.int32, device=self.device)
            scratch = torch.empty((PB * 32,), dtype=torch.int32, device=self.device)
            _check(lib.bsc_fb_table(base_t.data_ptr(), 0, 0, 1, 1, B0, NW, PB, 1, 0, self.table.data_ptr(),
                                    scratch.data_ptr(), S.raw()), "fb_table")
            torch.cuda.current_stream(self.device).synchronize()
            del scratch, base_t
        self._bufs: list = []    # every pinned read-back buffer made (sign)
        self._free: dict = {}    # capacity -> the ones no outstanding result uses

    def table_bytes(self) -> int:
        """The bytes of the table this signer built: 0 for a borrowed one."""
        return 0 if self.table is None or self.borrowed else self.table.numel() * 4

    def release(self) -> None:
        """Drop the table (a borrowed one: this reference to it); the signer is unusable afterwards.  Waits for the
        device: the read-back buffers go too."""
        if self.table is not None:
            torch.cuda.synchronize(self.device)   # no launch or read-back of this signer is in flight afterwards
        self.table = None
        self._bufs, self._free = [], {}

    # ------------------------------------------------------------------ launches
    def _upload(self, messages, msg_idx, key_idx, nonce_ids, sks, bases):
        msgs = np.ascontiguousarray(messages, np.uint8).reshape(-1, 64)
        mi = np.ascontiguousarray(msg_idx, np.int32).reshape(-1)
        ki = np.ascontiguousarray(key_idx, np.int32).reshape(-1)
        ids = (np.asarray(nonce_ids, np.int64).reshape(-1) & 0xffffffff).astype(np.uint32)
        n = int(mi.size)
        if not (ki.size == n and ids.size == n):
            raise ValueError("sign: msg_idx, key_idx and nonce_ids differ in length")
        if msgs.shape[0] < 1:
            raise ValueError("sign: at least one 64-byte message")
        sk_int = [_scalar_int(s) for s in sks]
        bs = [bytes(b) for b in bases]
        if not sk_int or len(bs) != len(sk_int) or any(len(b) != 32 for b in bs):
            raise ValueError("sign: at least one key, and one 32-byte nonce base per key")
        if any(not 0 <= s < self.order for s in sk_int):
            raise ValueError("sign: a secret key outside [0, n)")
        # sk 2^256 mod n, little-endian limbs: one Montgomery multiplication by c then gives sk c mod n
        keys = np.frombuffer(b"".join(((s << 256) % self.order).to_bytes(32, "little") for s in sk_int),
                             np.uint32).reshape(-1, 8)
        return msgs, mi, ki, ids, keys, np.frombuffer(b"".join(bs), np.uint8).reshape(-1, 32), sk_int, n

    def _launch(self, msgs, mi, ki, ids, keys, bs, n, counter):
        """-> (out int32 [17 cap] on the device: cap rows of 16 signature words, then cap statuses; cap)."""
        cap = max(256, (n + 255) & ~255)
        out = torch.empty((17 * cap,), dtype=torch.int32, device=self.device)
        if n == 0:
            return out, cap
        d_msgs, d_mi, d_ki, d_ids, d_keys, d_bs = h2d_many(
            [(msgs, torch.uint8), (mi, torch.int32), (ki, torch.int32), (ids.view(np.int32), torch.int32),
             (keys.view(np.int32), torch.int32), (bs, torch.uint8)], self.device)
        _check(hip().bsc_schnorr_sign(d_msgs.data_ptr(), d_mi.data_ptr(), d_ki.data_ptr(), d_ids.data_ptr(),
                                      d_keys.data_ptr(), d_bs.data_ptr(), self.table.data_ptr(), int(keys.shape[0]),
                                      int(msgs.shape[0]), n, out.data_ptr(), out.data_ptr() + 64 * cap,
                                      counter.data_ptr() if counter is not None else None, S.raw()), "schnorr_sign")
        return out, cap

    def launch(self, messages, msg_idx, key_idx, nonce_ids, sks, bases, counter=None):
        """Upload and launch on the current stream; nothing is read back: (sigs uint8 [n, 64], status int32 [n]) on
        the device.  counter: optional device int32 [1], incremented once per item whose status is not 0."""
        if self.table is None:
            raise RuntimeError("SchnorrSigner: released")
        msgs, mi, ki, ids, keys, bs, _, n = self._upload(messages, msg_idx, key_idx, nonce_ids, sks, bases)
        out, cap = self._launch(msgs, mi, ki, ids, keys, bs, n, counter)
        return out[:16 * n].view(torch.uint8).view(n, 64), out[16 * cap:16 * cap + n]

    def _host_buffer(self, words: int) -> torch.Tensor:
        """A pinned int32 [words] read-back buffer that no outstanding result uses (SchnorrVerifier._host_buffer)."""
        free = self._free.setdefault(words, [])
        if free:
            return free.pop()
        buf = torch.empty((words,), dtype=torch.int32, pin_memory=True)
        self._bufs.append(buf)
        return buf

    def sign(self, messages, msg_idx, key_idx, nonce_ids, sks, bases, counter=None):
        """One launch and one read-back on the current stream.  messages: uint8 [nmsg, 64]; msg_idx, key_idx,
        nonce_ids: int [n]; sks: the local signers' secret keys (32 big-endian bytes or int each); bases: their
        32-byte nonce bases.  Returns a callable giving (sigs uint8 [n, 64], status int32 [n]) (it waits for the
        read-back; call it once), with .ready and .inputs.  Any number of results may be outstanding."""
        if self.table is None:
            raise RuntimeError("SchnorrSigner: released")
        msgs, mi, ki, ids, keys, bs, sk_int, n = self._upload(messages, msg_idx, key_idx, nonce_ids, sks, bases)
        inputs = (msgs, mi, ki, ids, sk_int, bs)
        if n == 0:
            result = lambda: (np.zeros((0, 64), np.uint8), np.zeros(0, np.int32))   # noqa: E731
            result.ready = lambda: True
            result.inputs = inputs
            return result
        out, cap = self._launch(msgs, mi, ki, ids, keys, bs, n, counter)
        host = self._host_buffer(17 * cap)
        d2h_into(host, out)
        ev = S.record()
        box = [host, out]   # the device rows live until the copy has been waited for

        def result():
            S.host_wait(ev)
            if box[0] is None:
                raise RuntimeError("SchnorrSigner: a result is read once")
            words = box[0].numpy()
            sigs = words[:16 * n].copy().view(np.uint8).reshape(n, 64)
            status = words[16 * cap:16 * cap + n].copy()
            self._free[int(box[0].shape[0])].append(box[0])   # the copy has landed and been taken: reusable
            box[0] = box[1] = None
            return sigs, status
        result.ready = ev.query
        result.inputs = inputs   # the host arrays as uploaded (msgs, msg_idx, key_idx, nonce ids, keys, bases)
        return result

    def resolved(self, wait):
        """A sign() result with every status 3 signed by the host: a callable giving (sigs, status, replaced), the
        replaced items' status set to 0."""
        msgs, mi, ki, ids, sk_int, bs = wait.inputs

        def result():
            sigs, st = wait()
            which = np.flatnonzero(st == UNDECIDED)
            for i in which:
                k = int(ki[i])
                ent = bs[k].tobytes() + int(ids[i]).to_bytes(4, "little")
                sigs[i] = np.frombuffer(rt().schnorr_sign(msgs[mi[i]].tobytes(), sk_int[k].to_bytes(32, "big"), ent),
                                        np.uint8)
                st[i] = VALID
            return sigs, st, int(which.size)
        result.ready = wait.ready
        return result

    def sign_resolved(self, messages, msg_idx, key_idx, nonce_ids, sks, bases, counter=None):
        """sign() with every status-3 item replaced by ``rt().schnorr_sign(msg, sk, base + le32(id))``: a callable
        giving (sigs, status, replaced)."""
        return self.resolved(self.sign(messages, msg_idx, key_idx, nonce_ids, sks, bases, counter))

    # ------------------------------------------------------------------ the test entry points
    def nonce(self, entropy):
        """bsc_schnorr_nonce: entropy uint8 [n, 36] (base || le32(id)) -> (scalar uint8 [n, 32] big-endian, draws
        int32 [n]); draws 0 and a zero scalar where none of DRAWS candidates fits.  Synchronous."""
        e = np.array(entropy, np.uint8).reshape(-1, 36)
        n = e.shape[0]
        d_e = torch.from_numpy(e).to(self.device)
        sc = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        dr = torch.zeros((n,), dtype=torch.int32, device=self.device)
        _check(hip().bsc_schnorr_nonce(d_e.data_ptr(), n, sc.data_ptr(), dr.data_ptr(), S.raw()), "schnorr_nonce")
        return sc.cpu().numpy(), dr.cpu().numpy()

    def response(self, vs, sks, cs):
        """bsc_schnorr_response: vs, sks, cs ints below n -> [(v - sk c) mod n] as ints.  The keys go up as
        sk 2^256 mod n, as in sign().  Synchronous."""
        n = len(vs)
        assert len(sks) == n and len(cs) == n
        be = lambda xs: np.frombuffer(b"".join(int(x).to_bytes(32, "big") for x in xs), np.uint8).reshape(n, 32)   # noqa: E731
        skr = np.frombuffer(b"".join(((int(s) << 256) % self.order).to_bytes(32, "little") for s in sks),
                            np.int32).reshape(n, 8)
        d_v, d_k, d_c = (torch.from_numpy(a.copy()).to(self.device) for a in (be(vs), skr, be(cs)))
        out = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        _check(hip().bsc_schnorr_response(d_v.data_ptr(), d_k.data_ptr(), d_c.data_ptr(), n, out.data_ptr(),
                                          S.raw()), "schnorr_response")
        return [int.from_bytes(row.tobytes(), "big") for row in out.cpu().numpy()]


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
