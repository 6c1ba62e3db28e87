"""Schnorr signing on the GPU (kernels/schnorr.hip k_schnorr_sign, ops/schnorr.py SchnorrSigner) against the host
signer: the two test entry points (nonce, response), the case set of tests/_schnorr_sign_cases.py in one launch and
at the 16-item workgroup edges, out-of-range indices, the launcher's argument checks, outstanding results, the host's
resolution of status 3, and the engine with engine.sign_device on the waited and on the deferred path."""
import random

import numpy as np
import pytest
import torch

from _schnorr_sign_cases import be32, cases, entropy

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def signer():
    from biscotti_amd.ops.schnorr import SchnorrSigner

    sg = SchnorrSigner(DEV)
    assert sg.table_bytes() == 33 * 128 * 64
    yield sg
    sg.release()


def _arrays(items):
    cs = cases()
    msgs = np.frombuffer(b"".join(cs["messages"]), np.uint8).reshape(-1, 64)
    mi = np.asarray([it.msg_idx for it in items], np.int32)
    ki = np.asarray([it.key_idx for it in items], np.int32)
    ids = np.asarray([it.nonce_id for it in items], np.int64)
    return msgs, mi, ki, ids, [be32(s) for s in cs["sks"]], cs["bases"]


def _check_signed(items, sigs, status):
    from biscotti_amd.native import rt

    R = rt()
    cs = cases()
    assert status.tolist() == [0] * len(items)
    for it, row in zip(items, sigs):
        want = R.schnorr_sign(cs["messages"][it.msg_idx], be32(cs["sks"][it.key_idx]),
                              entropy(cs["bases"][it.key_idx], it.nonce_id))
        assert row.tobytes() == bytes(want), it
        assert R.schnorr_verify(cs["messages"][it.msg_idx], R.g1_base_mul(cs["sks"][it.key_idx]), row.tobytes()), it


# ---------------------------------------------------------------------------- the test entry points (run first)
def test_nonce_entry_point(signer):
    cs = cases()
    items = cs["items"]
    ent = np.frombuffer(b"".join(entropy(cs["bases"][it.key_idx], it.nonce_id) for it in items), np.uint8)
    sc, dr = signer.nonce(ent)
    assert dr.tolist() == [it.vdraws for it in items]
    assert [bytes(r) for r in sc] == [be32(it.v) for it in items]
    assert max(dr) >= 3   # the multi-draw cases are in


def test_response_entry_point(signer):
    n = cases()["order"]
    rnd = random.Random(12)
    vals = [1, 2, n - 2, n - 1, 2 ** 255] + [rnd.randrange(1, n) for _ in range(4)]
    vs, sks, cc = [], [], []
    for v in vals:
        for sk in vals:
            for c in vals:
                vs.append(v), sks.append(sk), cc.append(c)
    for sk in vals:          # r = 0 and r = n - 1
        for c in vals:
            vs.append(sk * c % n), sks.append(sk), cc.append(c)
            vs.append((sk * c - 1) % n), sks.append(sk), cc.append(c)
    got = signer.response(vs, sks, cc)
    want = [(v - sk * c) % n for v, sk, c in zip(vs, sks, cc)]
    assert got == want
    assert 0 in want and n - 1 in want


# ---------------------------------------------------------------------------- the kernel
def test_every_case_in_one_launch(signer):
    items = cases()["items"]
    sigs, status = signer.sign(*_arrays(items))()
    assert sigs.shape == (len(items), 64) and sigs.dtype == np.uint8
    _check_signed(items, sigs, status)
    assert [row.tobytes() for row in sigs] == [it.sig for it in items]   # and the integer model's bytes


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 65])
def test_workgroup_edges(signer, batch):
    items = cases()["items"]
    for lo in (0, len(items) - batch):
        part = items[lo:lo + batch]
        sigs, status = signer.sign(*_arrays(part))()
        assert [row.tobytes() for row in sigs] == [it.sig for it in part]
        assert status.tolist() == [0] * batch


def test_workgroup_mixing_valid_and_out_of_range(signer):
    cs = cases()
    items = cs["items"][:16]
    msgs, mi, ki, ids, sks, bases = _arrays(items)
    nmsg, nkeys = msgs.shape[0], len(sks)
    bad = {1: ("m", -1), 4: ("k", -1), 7: ("m", nmsg), 8: ("k", nkeys), 15: ("k", -1)}
    for i, (what, val) in bad.items():
        (mi if what == "m" else ki)[i] = val
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    sigs, status = signer.sign(msgs, mi, ki, ids, sks, bases, counter)()
    assert status.tolist() == [4 if i in bad else 0 for i in range(16)]
    for i in range(16):
        assert sigs[i].tobytes() == (bytes(64) if i in bad else items[i].sig)
    assert int(counter.item()) == len(bad)


def test_rejected_launcher_arguments_write_nothing(signer):
    from biscotti_amd.native import hip

    lib = hip()
    items = cases()["items"][:8]
    msgs, mi, ki, ids, sks, bases = _arrays(items)
    _, _, _, ids32, keys, bs, _, _ = signer._upload(msgs, mi, ki, ids, sks, bases)
    d = [torch.from_numpy(np.array(a)).to(DEV) for a in (msgs, mi, ki, ids32.view(np.int32), keys.view(np.int32), bs)]
    sigs = torch.full((8 * 64 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    counter = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    tbl, nk, nm = signer.table.data_ptr(), len(sks), msgs.shape[0]

    def call(msgs_p=d[0].data_ptr(), mi_p=d[1].data_ptr(), ki_p=d[2].data_ptr(), id_p=d[3].data_ptr(),
             key_p=d[4].data_ptr(), bs_p=d[5].data_ptr(), tbl_p=tbl, nkeys=nk, nmsg=nm, n=8, sg_p=sigs.data_ptr(),
             st_p=status.data_ptr()):
        return lib.bsc_schnorr_sign(msgs_p, mi_p, ki_p, id_p, key_p, bs_p, tbl_p, nkeys, nmsg, n, sg_p, st_p,
                                    counter.data_ptr(), None)

    assert call(n=-1) == -1 and call(nkeys=0) == -1 and call(nmsg=0) == -1
    for k in ("msgs_p", "mi_p", "ki_p", "id_p", "key_p", "bs_p", "tbl_p", "sg_p", "st_p"):
        assert call(**{k: None}) == -1, k
    for k, t in (("msgs_p", d[0]), ("bs_p", d[5]), ("sg_p", sigs)):   # a byte buffer off its 4-byte alignment
        assert call(**{k: t.data_ptr() + 1}) == -1, k
    assert call(n=0) == 0
    assert lib.bsc_schnorr_nonce(None, 4, sigs.data_ptr(), status.data_ptr(), None) == -1
    assert lib.bsc_schnorr_nonce(d[5].data_ptr(), -1, sigs.data_ptr(), status.data_ptr(), None) == -1
    assert lib.bsc_schnorr_response(d[5].data_ptr(), None, d[5].data_ptr(), 4, sigs.data_ptr(), None) == -1
    assert lib.bsc_schnorr_response(d[5].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 4, sigs.data_ptr() + 2,
                                    None) == -1
    torch.cuda.synchronize()
    assert set(sigs.tolist()) == {0xA5} and status.tolist() == [-7] * 8 and counter.tolist() == [-7]
    assert call() == 0   # and the same arguments, all valid, do launch
    torch.cuda.synchronize()
    assert status.tolist() == [0] * 8 and counter.tolist() == [-7]
    assert bytes(sigs[:512].tolist()) == b"".join(it.sig for it in items)
    assert sigs[512:].tolist() == [0xA5] * 4   # nothing past the eighth row


def test_outstanding_results_read_in_any_order(signer):
    items = cases()["items"]
    parts = [items[0:20], items[20:21], items[21:60], items[60:90]]
    waits = [signer.sign(*_arrays(p)) for p in parts]
    for k in (2, 0, 3, 1):
        sigs, status = waits[k]()
        assert [row.tobytes() for row in sigs] == [it.sig for it in parts[k]]
        assert not status.any()
    with pytest.raises(RuntimeError):
        waits[0]()   # a result is read once
    assert all(w.ready() for w in waits)


def test_sign_resolved_signs_a_status_3_item_on_the_host(signer):
    items = cases()["items"][10:30]
    sigs, status, replaced = signer.sign_resolved(*_arrays(items))()
    assert replaced == 0 and not status.any()
    wait = signer.sign(*_arrays(items))

    def forced():   # what the kernel leaves at the draw cap: status 3 and zero bytes
        sg, st = wait()
        st[7] = 3
        sg[7] = 0
        return sg, st
    forced.ready, forced.inputs = wait.ready, wait.inputs
    sigs2, status2, replaced2 = signer.resolved(forced)()
    assert replaced2 == 1 and not status2.any()
    assert (sigs2 == sigs).all() and sigs2[7].tobytes() == items[7].sig


def test_borrowed_table_signs_the_same_bytes():
    from biscotti_amd.native import rt
    from biscotti_amd.ops.schnorr import SchnorrSigner, SchnorrVerifier

    cs = cases()
    items = cs["items"][:17]
    sv = SchnorrVerifier([rt().g1_base_mul(s) for s in cs["sks"][:3]], DEV)
    sg = SchnorrSigner(DEV, table=sv)
    try:
        assert sg.table_bytes() == 0
        sv.release()   # the signer's reference keeps the table
        sigs, status = sg.sign(*_arrays(items))()
        assert [row.tobytes() for row in sigs] == [it.sig for it in items] and not status.any()
    finally:
        sg.release()


# ---------------------------------------------------------------------------- the engine
def _engine_run(cfg_kw: dict, rounds: int, sign_device: bool):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(max_iterations=100, deterministic_time=True, **cfg_kw)
    eng = BiscottiEngine(cfg, Comm(device=DEV))
    sigs = {}
    audit_seen = []

    def seam(sig_np, it):   # where a batch is joined: the round's signature matrix
        audit_seen.append(it)
        sigs[it] = sig_np.copy()
    try:
        eng.sign_device = sign_device
        if cfg.sig_audit:
            eng.sig_audit_tamper = seam
        res = []
        for i in range(rounds):
            res.append(eng.run_round(remaining=rounds - i))
            if not cfg.sig_audit:
                sigs[i] = eng.last_signatures.copy()
        eng.drain()
        return {"hashes": [r.block_hash for r in res], "nodes": [sorted(r.node_list) for r in res],
                "sigs": sigs, "stats": dict(eng.stats), "signer": eng._sign_dev is not None}
    finally:
        eng.close()


def test_engine_verify_signatures_with_the_device_signer():
    kw = dict(num_nodes=12, dataset="creditcard", seed=6, verify_signatures=True)
    off = _engine_run(kw, 3, False)
    on = _engine_run(kw, 3, True)
    assert not off["signer"] and not any(k.startswith("sign_") for k in off["stats"])
    assert on["signer"]
    assert on["hashes"] == off["hashes"] and on["nodes"] == off["nodes"] and len(set(on["hashes"])) == 3
    assert on["sigs"].keys() == off["sigs"].keys()
    for k in off["sigs"]:
        assert off["sigs"][k].any() and (on["sigs"][k] == off["sigs"][k]).all(), k
    assert on["stats"]["sign_device"] > 0 and on["stats"]["sign_device_host"] == 0
    assert on["stats"]["sig_failures"] == off["stats"]["sig_failures"] == 0
    assert on["stats"]["sig_checks"] == off["stats"]["sig_checks"] > 0


def test_engine_deferred_joins_with_the_device_signer():
    """MNIST on the pipelined path: the batches are deferred (the low-priority stream) and joined up to two rounds
    later; --sig-audit sees every joined batch."""
    kw = dict(num_nodes=20, dataset="mnist", seed=2, sig_audit=True)
    off = _engine_run(kw, 5, False)
    on = _engine_run(kw, 5, True)
    assert on["hashes"] == off["hashes"] and on["nodes"] == off["nodes"]
    assert sorted(on["sigs"]) == sorted(off["sigs"]) and len(on["sigs"]) == 5
    for k in off["sigs"]:
        assert off["sigs"][k].any() and (on["sigs"][k] == off["sigs"][k]).all(), k
    st = on["stats"]
    assert st["sig_audit_failures"] == 0 and off["stats"]["sig_audit_failures"] == 0
    assert st["sign_device"] > 0
    assert st["sig_audit_checked"] == st["sign_device"] + st["sign_device_host"] == off["stats"]["sig_audit_checked"]
    assert st["sign_table_bytes"] == 0 and st["sig_table_bytes"] > 0   # the verifier's table of G is shared
