"""Device ECVRF verifier (kernels/vrf.hip k_vrf_verify, ops/vrf.py) against the plain-Python verifier
(_ecvrf_verify_ref.py, pinned to RFC 9381 and to the host in test_vrf_verify_ref.py) and, for validity and the
output, against the host runtime's vrf_verify; then the prover's in-place audit and the engine's.

Inputs come from test_vrf_edges.py; the reference proofs are computed once per session (V.expected) and shared
with test_gpu_vrf.py."""
import numpy as np
import pytest
import torch

import _ecvrf_ref as E
import _ecvrf_verify_ref as VR
import test_vrf_edges as V

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SPARE = 16   # rows past n in status, beta and scratch that a launch must leave alone


@pytest.fixture(scope="module")
def btab(rt):
    return torch.from_numpy(np.frombuffer(rt.vrf_base_table(), np.int32).copy()).to("cuda")


def _direct(btab, keybuf: bytes, stride: int, off: int, pk_idx, alphas, alpha_idx, alpha_len, n, pis, expect=None,
            expect_idx=None, urgent=0):
    """One call of bsc_vrf_verify.  keybuf: the key buffer (bytes); key i is the 8 words at word off +
    pk_idx[i] * stride.  Returns (return value, statuses, beta rows, counter) after a sync, and checks that
    nothing past row n of status, beta or scratch was written."""
    from biscotti_amd.native import hip
    from biscotti_amd.utils import streams as S
    # the kernel trusts its indices: keep every read in bounds (a launch also reads entry 0 of the index arrays)
    assert len(keybuf) % 4 == 0 and len(pk_idx) == len(alpha_idx) >= max(n, 1) and len(pis) >= max(n, 1)
    assert 0 <= min(pk_idx) and 4 * (off + max(pk_idx) * stride + 8) <= len(keybuf)
    assert 0 <= min(alpha_idx) and max(alpha_idx) < len(alphas) and all(len(p) == 80 for p in pis)
    assert not 0 <= alpha_len <= 1024 or all(len(a) == alpha_len for a in alphas)
    dev = "cuda"
    m = max(n, 0) + SPARE
    keys = torch.from_numpy(np.frombuffer(keybuf, np.int32).copy()).to(dev)
    al = torch.from_numpy(np.frombuffer(b"".join(alphas) + b"\x00", np.uint8).copy()).to(dev)
    kidx = torch.tensor(list(pk_idx), dtype=torch.int32, device=dev)
    aidx = torch.tensor(list(alpha_idx), dtype=torch.int32, device=dev)
    pi = torch.from_numpy(np.frombuffer(b"".join(pis), np.uint8).copy()).to(dev)
    ex = eidx = None
    if expect is not None:
        assert len(expect_idx) >= max(n, 1) and -1 <= min(expect_idx) and max(expect_idx) < len(expect)
        ex = torch.from_numpy(np.frombuffer(b"".join(expect), np.uint8).copy()).to(dev)
        eidx = torch.tensor(list(expect_idx), dtype=torch.int32, device=dev)
    status = torch.full((m, 4), SENTINEL, dtype=torch.uint8, device=dev)
    bt = torch.full((m, 64), SENTINEL, dtype=torch.uint8, device=dev)
    scratch = torch.full((m, 960 * 4), SENTINEL, dtype=torch.uint8, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    ret = hip().bsc_vrf_verify(keys.data_ptr() + 4 * off, stride, kidx.data_ptr(), al.data_ptr(), aidx.data_ptr(),
                               alpha_len, n, btab.data_ptr(), scratch.data_ptr(), pi.data_ptr(),
                               ex.data_ptr() if ex is not None else None,
                               eidx.data_ptr() if eidx is not None else None, status.data_ptr(), bt.data_ptr(),
                               counter.data_ptr(), urgent, S.raw())
    torch.cuda.synchronize()
    status, bt, scratch = status.cpu().numpy(), bt.cpu().numpy(), scratch.cpu().numpy()
    k = max(n, 0) if ret == 0 else 0
    assert (status[k:] == SENTINEL).all() and (bt[k:] == SENTINEL).all() and (scratch[k:] == SENTINEL).all()
    return ret, status[:k].copy().view(np.int32).reshape(-1).tolist(), [bytes(r) for r in bt[:k]], int(counter.item())


def _packed(btab, triples, alpha_len=32, **kw):
    """(pk, alpha, pi) triples through the direct call with packed 8-word keys."""
    pks = list(dict.fromkeys(t[0] for t in triples))
    als = list(dict.fromkeys(t[1] for t in triples))
    return _direct(btab, b"".join(pks), 8, 0, [pks.index(t[0]) for t in triples], als,
                   [als.index(t[1]) for t in triples], alpha_len, len(triples), [t[2] for t in triples], **kw)


def _valid_triples(pairs):
    return [(E.key_from_seed(s)[2], a, V.expected(s, a)[0]) for s, a in pairs]


def _all_valid(btab, pairs, alpha_len=32):
    ret, status, beta, fails = _packed(btab, _valid_triples(pairs), alpha_len)
    assert ret == 0 and status == [0] * len(pairs) and fails == 0
    for i, (s, a) in enumerate(pairs):
        assert beta[i] == V.expected(s, a)[1], i


# ------------------------------------------------------------------------------------------- the kernel
def test_tamper_set_in_one_launch(rt, btab):
    """All 640 single-bit flips of one proof and the named cases: statuses and outputs row by row."""
    cases, ref = VR.cases(), VR.reference()
    ret, status, beta, fails = _packed(btab, [c[1:] for c in cases])
    assert ret == 0 and len(status) == len(cases) >= VR.N_FLIPS + 30
    for i, ((name, pk, alpha, pi), (st, b)) in enumerate(zip(cases, ref)):
        assert status[i] == st, name
        assert beta[i] == b, name
        host = rt.vrf_verify(pk, alpha, pi)
        assert (host is None) == (status[i] != 0) and (host is None or host == beta[i]), name
        if status[i] != 0:
            assert beta[i] == bytes(64), name
    assert fails == sum(1 for s in status if s != 0) > VR.N_FLIPS
    assert {0, 1, 2, 3, 4} <= set(status)


def test_rfc9381_vector(btab):
    _, pk, alpha, pi = VR.rfc_case()
    ret, status, beta, fails = _packed(btab, [(pk, alpha, pi)], alpha_len=0)
    assert (ret, status, fails) == (0, [0], 0) and beta[0].hex() == V.RFC_BETA


def test_valid_proofs_with_counters_of_12_and_more(btab):
    """First counters 0..17 mixed in one workgroup, then 16 proofs that all need the second pass."""
    _all_valid(btab, V.inputs_counter_mix())
    _all_valid(btab, V.inputs_counter_high())


@pytest.mark.parametrize("alpha_len", V.ALPHA_LENS)
def test_valid_proofs_at_block_edge_lengths(btab, alpha_len):
    pairs = [(s, a) for s, a in V.inputs_lens() if len(a) == alpha_len]
    assert len(pairs) == len(V.LEN_KEY_IDX)
    _all_valid(btab, pairs, alpha_len)


@pytest.mark.parametrize("n", V.BATCH_NS)
def test_batch_sizes_and_partial_workgroups(btab, n):
    """n around the 16 proofs of a workgroup: the lanes past n write nothing (_direct's sentinel rows); the
    result does not depend on urgent."""
    pairs = V.inputs_batch()[:n]
    _all_valid(btab, pairs)
    tr = _valid_triples(pairs)
    assert _packed(btab, tr, urgent=1) == _packed(btab, tr)


def test_rejected_arguments_write_nothing(btab):
    tr = _valid_triples(V.inputs_batch()[:5])
    pks = b"".join(t[0] for t in tr)
    for alpha_len in (-1, 1025):
        ret, status, beta, fails = _direct(btab, pks, 8, 0, range(5), [bytes(2048)], [0] * 5, alpha_len, 5,
                                           [t[2] for t in tr])   # _direct checks the sentinels
        assert (ret, status, beta, fails) == (-1, [], [], 0)
    for n in (0, -3):
        ret, status, beta, fails = _direct(btab, pks, 8, 0, range(5), [bytes(32)], [0] * 5, 32, n, [t[2] for t in tr])
        assert (ret, status, beta, fails) == (0, [], [], 0)


def test_workgroup_mixing_valid_and_invalid_proofs(btab):
    """16 rows alternating valid / Gamma undecodable / s >= L / wrong key: the failing proofs stop working but
    walk the barriers, so the valid rows of their workgroup come out as they do alone."""
    base = _valid_triples(V.inputs_batch()[:16])
    p1 = (E.P + 1).to_bytes(32, "little")
    rows, want = [], []
    for i, (pk, a, pi) in enumerate(base):
        if i % 4 == 1:
            pi = p1 + pi[32:]
        elif i % 4 == 2:
            pi = pi[:48] + (int.from_bytes(pi[48:], "little") + E.L).to_bytes(32, "little")
        elif i % 4 == 3:
            pk = base[(i + 1) % 16][0]
        rows.append((pk, a, pi))
        want.append([0, 2, 3, 4][i % 4])
    ret, status, beta, fails = _packed(btab, rows)
    assert ret == 0 and status == want and fails == 12
    for i, (s, a) in enumerate(V.inputs_batch()[:16]):
        assert beta[i] == (V.expected(s, a)[1] if i % 4 == 0 else bytes(64)), i
        assert VR.verify(*rows[i])[0] == want[i]


def test_expected_outputs(btab):
    """The right output: 0; another proof's: 5 (the output is still written); index -1: 0; a failing proof stays
    at its own status."""
    pairs = V.inputs_batch()[:6]
    tr = _valid_triples(pairs)
    betas = [V.expected(s, a)[1] for s, a in pairs]
    tr[5] = (tr[5][0], tr[5][1], tr[5][2][:40] + bytes([tr[5][2][40] ^ 1]) + tr[5][2][41:])
    expect_idx = [0, 2, -1, 3, 3, 4]     # proof 1 against proof 2's output, proof 4 against proof 3's
    ret, status, beta, fails = _packed(btab, tr, expect=betas, expect_idx=expect_idx)
    assert ret == 0 and status == [0, 5, 0, 0, 5, 4] and fails == 3
    assert beta[:5] == betas[:5] and beta[5] == bytes(64)


def test_key_stride_packed_rows_and_prover_rows(rt, btab):
    """The same keys from packed 8-word rows and from the prover's 96-byte rows (keys + 16, stride 24); with the
    secret and the nonce prefix of every row overwritten, so only the 8 key words can have been read."""
    pairs = V.inputs_batch()[:17]
    tr = _valid_triples(pairs)
    tr[3] = (tr[3][0], tr[3][1], tr[4][2])   # one failure, so the two runs agree on more than zeros
    als = list(dict.fromkeys(t[1] for t in tr))
    aidx = [als.index(t[1]) for t in tr]
    packed = _direct(btab, b"".join(t[0] for t in tr), 8, 0, range(17), als, aidx, 32, 17, [t[2] for t in tr])
    for filler in (None, b"\xEE" * 64):
        rows = b"".join((rt.vrf_key_material(s)[:64] if filler is None else filler) + t[0]
                        for (s, _), t in zip(pairs, tr))
        assert _direct(btab, rows, 24, 16, range(17), als, aidx, 32, 17, [t[2] for t in tr]) == packed
    assert packed[1] == [0, 0, 0, 4] + [0] * 13 and packed[3] == 1


# ------------------------------------------------------------------------------------------- the wrapper
def test_wrapper_verify(rt):
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda")
    cases, ref = VR.cases()[VR.N_FLIPS:], VR.reference()[VR.N_FLIPS:]
    status, beta = prover.verify([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [st for st, _ in ref]
    assert [bytes(r) for r in beta.cpu().numpy()] == [b for _, b in ref]
    ok = [(c, b) for c, (st, b) in zip(cases, ref) if st == 0][:3]
    status, _ = prover.verify([c[1] for c, _ in ok], [c[2] for c, _ in ok], [c[3] for c, _ in ok],
                              expect=[ok[0][1], None, ok[0][1]])
    assert status.cpu().tolist() == [0, 0, 5]
    _, pk, alpha, pi = VR.rfc_case()
    status, beta = prover.verify([pk], [alpha], [pi])
    assert status.cpu().tolist() == [0] and bytes(beta.cpu().numpy()[0]).hex() == V.RFC_BETA
    assert prover.verify([], [], [])[0].shape == (0,)
    for bad in (([pk[:31]], [alpha], [pi]), ([pk], [alpha], [pi[:79]]), ([pk, pk], [alpha, b"x"], [pi, pi]),
                ([pk], [bytes(1025)], [pi]), ([pk], [alpha, alpha], [pi])):
        with pytest.raises(ValueError):
            prover.verify(*bad)
    with pytest.raises(ValueError):
        prover.verify([pk], [alpha], [pi], expect=[b"short"])


def _audited_rounds(tamper=None):
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda", batch_rounds=2)
    prover.audit = True
    prover.audit_tamper = tamper
    st = torch.cuda.Stream()
    for r, (sl, a) in enumerate(V.WRAP_TWO):
        seeds = V.POOL_SEEDS[sl]
        # the first three proofs of a round carry their expected output
        expect = b"".join(V.expected(s, V.POOL_ALPHAS[a])[1] for s in seeds[:3])
        prover.submit(seeds, V.POOL_ALPHAS[a], st, expect=expect, tag=("round", r))
    assert prover.proofs == 37
    prover.drain(st)
    return prover.audit_result()


def test_prove_then_verify_in_place():
    """Two queued rounds (20 + 17 proofs, one prove launch) verified in the same buffers on the same stream."""
    assert _audited_rounds() == (37, 0, None)


def test_in_place_audit_sees_a_flipped_bit():
    def flip(pi, tags):
        assert tags == [("round", 0), ("round", 1)] and pi.shape == (37, 80)
        pi[20 + 5, 40] ^= 1   # proof 5 of the second round, a bit of c

    assert _audited_rounds(flip) == (37, 1, (("round", 1), 5, 4))


def test_one_round_flush_is_audited_too():
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda", batch_rounds=2)
    prover.audit = True
    st = torch.cuda.Stream()
    seeds, alpha = V.POOL_SEEDS[:21], V.POOL_ALPHAS[0]
    wrong = V.expected(seeds[1], alpha)[1] + V.expected(seeds[1], alpha)[1]   # proof 0 against proof 1's output
    prover.submit(seeds, alpha, st, expect=wrong, tag="only")
    prover.drain(st)
    assert prover.audit_result() == (21, 1, ("only", 0, 5))


# ------------------------------------------------------------------------------------------- the engine
ROUNDS = 4


def _engine_run(audit: bool, tamper=None):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine
    cfg = RunConfig(num_nodes=12, dataset="creditcard", seed=6, max_iterations=100, deterministic_time=True,
                    vrf_audit=audit)
    eng = BiscottiEngine(cfg, Comm(device=torch.device("cuda", 0)))
    try:
        prover = eng.vrf_dev
        prover.audit_tamper = tamper   # the audit's test seam (protocol/vrf_audit.py)
        # every batch the prover launches: (rounds done, urgent, proofs launched, proofs audited so far)
        launches, flush = [], prover.flush

        def recorded(stream, urgent=False):
            queued = sum(int(e[0].size) for e in prover._queue)
            flush(stream, urgent=urgent)
            if queued:
                launches.append((eng.rounds_done, bool(urgent), queued, prover.audit_checked))

        prover.flush = recorded
        # (remaining: the penultimate round's front sends the queued proofs to the device at low priority, the
        # last round's are proved on the host -- the audit covers both)
        hashes = [eng.run_round(remaining=ROUNDS - i).block_hash for i in range(ROUNDS)]
        eng.drain()
        stats = dict(eng.stats)
        stats["launches"] = launches
        return hashes, stats
    finally:
        eng.close()


@pytest.fixture(scope="module")
def run_without_audit():
    hashes, stats = _engine_run(False)
    assert "vrf_audit_checked" not in stats
    return hashes, stats["launches"]


@pytest.fixture(scope="module")
def chain_without_audit(run_without_audit):
    return run_without_audit[0]


def test_engine_audit_checks_every_proof(run_without_audit):
    chain, launches = run_without_audit
    hashes, stats = _engine_run(True)
    print({k: v for k, v in stats.items() if "vrf" in k or k == "launches"})
    assert stats["vrf_audit_checked"] == stats["vrf_device_proofs"] + stats.get("vrf_host_proofs", 0) > 0
    assert stats["vrf_device_proofs"] > 0
    assert stats["vrf_audit_failures"] == 0
    assert hashes == chain
    # the audit follows the prover's batches, it does not move them: the same launches at the same points of
    # the run and at the same priority as with the audit off -- the penultimate round's low-priority flush, before
    # the last round, among them -- each audited in full as it is launched
    assert [x[:3] for x in stats["launches"]] == [x[:3] for x in launches]
    assert launches[0][1] is False and launches[0][0] < ROUNDS - 1
    assert [x[3] for x in stats["launches"]] == [sum(y[2] for y in launches[:i + 1]) for i in range(len(launches))]
    assert [x[3] for x in launches] == [0] * len(launches)


def test_engine_audit_counts_one_tampered_proof(chain_without_audit):
    done = []

    def flip(pi, tags):   # bit 0 of byte 40 of the first proof of iteration 1, once
        off = 0
        for it, peers in tags:
            if it == 1 and not done:
                done.append((it, peers[0]))
                pi[off, 40] ^= 1
            off += len(peers)
        assert off == pi.shape[0]

    hashes, stats = _engine_run(True, flip)
    assert done
    assert stats["vrf_audit_failures"] == 1
    assert stats["vrf_audit_checked"] == stats["vrf_device_proofs"] + stats.get("vrf_host_proofs", 0)
    assert hashes == chain_without_audit
