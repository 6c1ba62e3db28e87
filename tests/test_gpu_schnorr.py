"""Batched Schnorr verification on the GPU (kernels/schnorr.hip, ops/schnorr.py) against the host verifier:
the two test entry points (challenge, point sum), the case set of tests/_schnorr_cases.py in one launch and in
partial workgroups, the launcher's argument checks, the quorum helper, and the engine with --verify-signatures and
--sig-audit."""
import random

import numpy as np
import pytest
import torch

from _schnorr_cases import be32, cases, challenge, point

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def verifier():
    from biscotti_amd.ops.schnorr import SchnorrVerifier

    sv = SchnorrVerifier(cases()["keys"], DEV)
    yield sv
    sv.release()


def _arrays(items):
    cs = cases()
    msgs = np.frombuffer(b"".join(cs["messages"]), np.uint8).reshape(-1, 64)
    mi = np.asarray([c.msg_idx for c in items], np.int32)
    ki = np.asarray([c.key_idx for c in items], np.int32)
    sg = np.frombuffer(b"".join(c.sig for c in items), np.uint8).reshape(-1, 64)
    want = np.asarray([c.expect for c in items], np.int32)
    return msgs, mi, ki, sg, want


# ---------------------------------------------------------------------------- the test entry points (run first)
def test_challenge_entry_point(verifier):
    from biscotti_amd.native import rt

    R = rt()
    n = R.bn256_order()
    rnd = random.Random(5)
    tms = [R.g1_base_mul(rnd.randrange(1, n)) for _ in range(62)] + [bytes(64), R.g1_generator()]
    msgs = [R.g1_base_mul(rnd.randrange(1, n)) for _ in range(63)] + [bytes(64)]
    want = [challenge(t, m) for t, m in zip(tms, msgs)]
    sc, dr = verifier.challenge(np.frombuffer(b"".join(tms), np.uint8), np.frombuffer(b"".join(msgs), np.uint8))
    assert dr.tolist() == [d for _, d in want]
    assert [bytes(r) for r in sc] == [be32(c) for c, _ in want]
    assert max(dr) > 1   # some pair needed more than one draw: the second candidate of a node is covered


def test_point_entry_point(verifier):
    cs = cases()
    n, keys = cs["order"], cs["keys"]
    rnd = random.Random(6)
    sc = list(cs["scalars"])
    # more digit edges, under ordinary keys: zero scalars, all-0x80 / all-0x81 bytes and the top bytes 0x81..0x8f on
    # both sides (the carry into window 32 of the key's table too)
    e80, e81 = int.from_bytes(b"\x80" * 32, "big"), int.from_bytes(b"\x81" * 32, "big")
    sc += [(0, 0, 0), (1, 0, 1), (0, 1, 2), (e80, e80, 3), (e81, e81, 4), (n - 1, n - 1, 5), (n - 1, 1, 6),
           (2 ** 255 - 1, 2 ** 255, 7), (0x8F << 248, 0x8F << 248, 0)]
    sc += [((0x81 + i) << 248 | rnd.getrandbits(240), (0x8F - i) << 248 | rnd.getrandbits(240), i % 8)
           for i in range(8)]
    sc += [(rnd.randrange(n), rnd.randrange(n), rnd.randrange(len(keys))) for _ in range(16)]
    sc = [(r % n, c % n, k) for r, c, k in sc]
    got = verifier.point(np.frombuffer(b"".join(be32(r) for r, _, _ in sc), np.uint8),
                         np.frombuffer(b"".join(be32(c) for _, c, _ in sc), np.uint8), [k for _, _, k in sc])
    want = [point(r, c, keys[k]) for r, c, k in sc]
    bad = [i for i, w in enumerate(want) if bytes(got[i]) != w]
    assert not bad, [(i, hex(sc[i][0]), hex(sc[i][1]), sc[i][2]) for i in bad]
    assert bytes(64) in want   # T = infinity is among them


def test_point_entry_point_key_out_of_range(verifier):
    got = verifier.point(np.frombuffer(be32(5) * 3, np.uint8), np.frombuffer(be32(7) * 3, np.uint8),
                         [-1, verifier.nkeys, 0])
    assert not got[0].any() and not got[1].any()
    assert bytes(got[2]) == point(5, 7, cases()["keys"][0])


# ---------------------------------------------------------------------------- the verifier
def test_case_set_in_one_launch(verifier):
    items = cases()["cases"]
    msgs, mi, ki, sg, want = _arrays(items)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = verifier.verify(msgs, mi, ki, sg, counter)()
    bad = [(items[i].name, int(st[i]), int(want[i])) for i in np.flatnonzero(st != want)]
    assert not bad, bad
    assert 3 not in st.tolist()
    assert int(counter.item()) == int((want != 0).sum())


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 65])
def test_case_set_in_batches(verifier, batch):
    """The whole set in launches of `batch` items, every result outstanding until all are launched (batch 1: one
    result per case, each alone in its workgroup)."""
    items = cases()["cases"]
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    waits = []
    for s in range(0, len(items), batch):
        msgs, mi, ki, sg, want = _arrays(items[s:s + batch])
        waits.append((verifier.verify(msgs, mi, ki, sg, counter), want))
    assert sum(len(w) for _, w in waits) == len(items)
    nonzero = 0
    for k, (wait, want) in enumerate(waits):
        assert wait().tolist() == want.tolist(), items[k * batch].name
        nonzero += int((want != 0).sum())
    assert nonzero > 0 and int(counter.item()) == nonzero


def test_results_read_in_any_order(verifier):
    """Every outstanding result has a read-back buffer of its own: read newest first, each gives its own launch's
    statuses; a result is read once."""
    items = cases()["cases"]
    waits = []
    for s in range(0, len(items), 7):
        msgs, mi, ki, sg, want = _arrays(items[s:s + 7])
        waits.append((verifier.verify(msgs, mi, ki, sg), want))
    assert len(waits) > 8 and len({tuple(w.tolist()) for _, w in waits}) > 2
    for wait, want in reversed(waits):
        assert wait().tolist() == want.tolist()
    with pytest.raises(RuntimeError):
        waits[0][0]()


def test_more_keys_than_one_table_build_launch():
    """40 keys: the table is built in two launches (32 bases each, G included); keys on both sides of the seam
    verify their own signatures and reject their neighbours'."""
    from biscotti_amd.native import rt
    from biscotti_amd.ops import schnorr as OS

    R = rt()
    n = R.bn256_order()
    rnd = random.Random(11)
    sks = [rnd.randrange(1, n) for _ in range(40)]
    assert 1 + len(sks) > OS._BUILD_BATCH
    msg = R.g1_base_mul(rnd.randrange(1, n))
    signers = [0, 29, 30, 31, 32, 33, 39]
    sigs = [R.schnorr_sign(msg, be32(sks[k]), rnd.randbytes(32)) for k in signers]
    sv = OS.SchnorrVerifier([R.g1_base_mul(s) for s in sks], DEV)
    try:
        ki = signers + [(k + 1) % 40 for k in signers]
        st = sv.verify(np.frombuffer(msg, np.uint8), [0] * len(ki), ki,
                       np.frombuffer(b"".join(sigs + sigs), np.uint8))()
        assert st.tolist() == [0] * len(signers) + [2] * len(signers)
    finally:
        sv.release()


def test_workgroup_mixing_valid_invalid_and_out_of_range(verifier):
    items = cases()["cases"]
    by = {e: [c for c in items if c.expect == e] for e in (0, 1, 2, 4)}
    mix = [by[(0, 2, 4, 0, 1, 0, 4, 2)[i % 8]][i // 8] for i in range(16)]
    msgs, mi, ki, sg, want = _arrays(mix)
    assert set(want.tolist()) == {0, 1, 2, 4}
    assert verifier.verify(msgs, mi, ki, sg)().tolist() == want.tolist()


def test_rejected_launcher_arguments_write_nothing(verifier):
    from biscotti_amd.native import hip

    lib = hip()
    items = cases()["cases"][:8]
    msgs, mi, ki, sg, _ = _arrays(items)
    d = [torch.from_numpy(np.array(a)).to(DEV) for a in (msgs, mi, ki, sg)]
    status = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    counter = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    tbl, nk, nm = verifier.table.data_ptr(), verifier.nkeys, msgs.shape[0]

    def call(msgs_p=d[0].data_ptr(), mi_p=d[1].data_ptr(), ki_p=d[2].data_ptr(), sg_p=d[3].data_ptr(), tbl_p=tbl,
             nkeys=nk, nmsg=nm, n=8, st_p=status.data_ptr()):
        return lib.bsc_schnorr_verify(msgs_p, mi_p, ki_p, sg_p, tbl_p, nkeys, nmsg, n, st_p, counter.data_ptr(), None)

    assert call(n=-1) == -1 and call(nkeys=0) == -1 and call(nmsg=0) == -1
    for k in ("msgs_p", "mi_p", "ki_p", "sg_p", "tbl_p", "st_p"):
        assert call(**{k: None}) == -1, k
    assert call(n=0) == 0
    assert lib.bsc_schnorr_challenge(None, d[0].data_ptr(), 4, status.data_ptr(), status.data_ptr(), None) == -1
    assert lib.bsc_schnorr_point(d[3].data_ptr(), d[3].data_ptr(), d[2].data_ptr(), tbl, 0, 4, d[0].data_ptr(),
                                 None) == -1
    torch.cuda.synchronize()
    assert status.tolist() == [-7] * 8 and counter.tolist() == [-7]
    assert call() == 0   # and the same arguments, all valid, do launch
    torch.cuda.synchronize()
    assert status.tolist() == [c.expect for c in items]


def test_verify_resolved_and_quorum_against_the_host_loop():
    from biscotti_amd.native import rt
    from biscotti_amd.ops.schnorr import SchnorrVerifier, quorum

    R = rt()
    n = R.bn256_order()
    rnd = random.Random(9)
    sks = [rnd.randrange(1, n) for _ in range(5)]
    pks = [R.g1_base_mul(s) for s in sks]
    plan = [3, 0, 4]                                   # the round's three verifiers among five peers
    workers = list(range(100, 120))
    commit = {w: R.g1_base_mul(rnd.randrange(1, n)) for w in workers}
    sigs = {}
    for w in workers:
        row = []
        for s in range(3):
            kind = rnd.randrange(4)
            signer = plan[s] if kind else 1            # kind 0: a peer outside the committee signed
            sg = R.schnorr_sign(commit[w], be32(sks[signer]), rnd.randbytes(32))
            if kind == 1:
                sg = sg[:50] + bytes([sg[50] ^ 4]) + sg[51:]
            row.append(sg)
        sigs[w] = row
    host = {w: sum(any(R.schnorr_verify(commit[w], pks[v], sg) for v in plan) for sg in sigs[w]) for w in workers}
    assert 0 in host.values() or 1 in host.values()
    sv = SchnorrVerifier(pks, DEV)
    try:
        mi, ki, rows, groups = [], [], [], []
        for m, w in enumerate(workers):
            for s, sg in enumerate(sigs[w]):
                for v in plan:
                    mi.append(m)
                    ki.append(v)
                    rows.append(sg)
                    groups.append((w, s))
        st = sv.verify_resolved(np.frombuffer(b"".join(commit[w] for w in workers), np.uint8), mi, ki,
                                np.frombuffer(b"".join(rows), np.uint8))()
        assert len(st) == 20 * 3 * 3 and set(st.tolist()) <= {0, 2}
        assert quorum(st, groups) == host
    finally:
        sv.release()


# ---------------------------------------------------------------------------- the engine
ROUNDS = 3


def _engine_run(host_loop: bool, tamper=None):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(num_nodes=12, dataset="creditcard", seed=6, max_iterations=100, deterministic_time=True,
                    verify_signatures=True)
    eng = BiscottiEngine(cfg, Comm(device=DEV))
    try:
        eng.sig_dev_off = host_loop
        eng.sig_tamper = tamper
        res = [eng.run_round(remaining=ROUNDS - i) for i in range(ROUNDS)]
        eng.drain()
        return [r.block_hash for r in res], [sorted(r.node_list) for r in res], dict(eng.stats), \
            eng._sig_dev is not None
    finally:
        eng.close()


def _corrupt(which):
    def tamper(signatures):   # each round's worker with the most signatures (the lowest such): all of them, or the first
        if signatures:
            w = max(signatures, key=lambda x: (len(signatures[x]), -x))
            sg = signatures[w]
            for s in range(len(sg) if which == "all" else 1):
                sg[s] = sg[s][:40] + bytes([sg[s][40] ^ 1]) + sg[s][41:]
    return tamper


@pytest.fixture(scope="module")
def untampered_host_loop():
    return _engine_run(True)


def test_engine_verify_signatures_matches_the_host_loop(untampered_host_loop):
    h_hash, h_nodes, h_stats, h_table = untampered_host_loop
    d_hash, d_nodes, d_stats, d_table = _engine_run(False)
    assert d_table and not h_table          # the device path built its tables, the host loop none
    assert d_hash == h_hash and d_nodes == h_nodes
    assert d_stats["sig_checks"] == h_stats["sig_checks"] > 0
    assert d_stats["sig_failures"] == h_stats["sig_failures"] == 0


@pytest.mark.parametrize("which", ["all", "one"])
def test_engine_verify_signatures_tampered_matches_the_host_loop(untampered_host_loop, which):
    h_hash, h_nodes, h_stats, _ = _engine_run(True, _corrupt(which))
    d_hash, d_nodes, d_stats, _ = _engine_run(False, _corrupt(which))
    assert d_hash == h_hash and d_nodes == h_nodes
    assert d_stats["sig_failures"] == h_stats["sig_failures"] > 0
    if which == "one":   # a worker with one bad signature of several keeps its place: the untampered chain
        assert d_hash == untampered_host_loop[0]
    else:                # a worker without a valid signature is dropped
        assert d_hash != untampered_host_loop[0]


def test_engine_sig_audit_on_gpu():
    from test_sig_audit_cpu import run_engine

    from biscotti_amd.parallel.comm import Comm

    off_hashes, off_stats, seen, lines = run_engine(False, device=None, comm=Comm(device=DEV))
    assert "sig_audit_checked" not in off_stats and "sig_table_bytes" not in off_stats and seen == 0
    hashes, stats, seen, lines = run_engine(True, device=None, comm=Comm(device=DEV))
    assert stats["sig_audit_checked"] == seen >= ROUNDS
    assert stats["sig_audit_failures"] == 0 and not lines and stats["sig_table_bytes"] > 0
    assert hashes == off_hashes
    done = []

    def flip(sig_np, it):
        if it == 1 and not done:
            v, j = [(int(a), int(b)) for a, b in zip(*sig_np.any(axis=2).nonzero())][0]
            sig_np[v, j, 40] ^= 1
            done.append((v, j))

    hashes, stats, seen, lines = run_engine(True, flip, device=None, comm=Comm(device=DEV))
    assert done and stats["sig_audit_checked"] == seen
    assert stats["sig_audit_failures"] == 1 and len(lines) == 1 and "iteration 1" in lines[0]
    assert hashes == off_hashes


def test_engine_sig_audit_with_deferred_joins():
    """MNIST rounds on the pipelined path: a round's signature batch is joined up to two rounds later, when the
    pinned commitment rows it signed belong to a later round -- the audit must check each signature against the
    message its signer read.  With room for two unread batches only, the audit reads its oldest ones while the run
    goes on; one flipped bit is found all the same, and nothing else."""
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(num_nodes=20, dataset="mnist", seed=2, max_iterations=100, deterministic_time=True,
                    sig_audit=True)
    eng = BiscottiEngine(cfg, Comm(device=DEV))
    done, seen = [], []

    def flip(sig_np, it):
        seen.append(int(sig_np.any(axis=2).sum()))
        if it == 2 and not done:
            v, j = [(int(a), int(b)) for a, b in zip(*sig_np.any(axis=2).nonzero())][0]
            sig_np[v, j, 7] ^= 16
            done.append((v, j))

    try:
        eng.sig_audit_keep = 2
        eng.sig_audit_tamper = flip
        for i in range(8):
            eng.run_round(remaining=8 - i)
        eng.drain()
        assert done and len(seen) == 8
        assert eng.stats["sig_audit_checked"] == sum(seen) >= 8
        assert eng.stats["sig_audit_failures"] == 1
        assert eng._sig_audit_acc["first"][0] == 2
    finally:
        eng.close()
