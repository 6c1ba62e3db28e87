"""Device ECVRF prover (kernels/vrf.hip) bit-exact against the host runtime (RFC 9381 pinned in
test_crypto.py::test_ecvrf_rfc9381_vector): proofs, outputs, verification, round-batched queue.

The edge tests below compare with the plain-Python reference (_ecvrf_ref.py, pinned to the RFC and to the host
in test_vrf_edges.py, which also holds the inputs): hash-to-curve counters of 12 and more, crafted secret
scalars, message lengths at the SHA-512 block edges, partial workgroups, and the wrapper's upload paths.
A hash whose y is non-canonical (about 2^-250) and a pair with no decoding counter (2^-256) cannot be reached
by any input and are not covered."""
import numpy as np
import pytest
import torch

import _ecvrf_ref as E
import test_vrf_edges as V

pytestmark = pytest.mark.gpu


def test_device_vrf_proofs_match_host(rt):
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda")
    rng = np.random.default_rng(3)
    seeds = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(150)]
    alphas = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(32), b"\xff" * 32]
    al = [alphas[i % 3] for i in range(len(seeds))]
    pi, beta = prover.prove(seeds, al, beta=True)
    torch.cuda.synchronize()
    pi, beta = pi.cpu().numpy(), beta.cpu().numpy()
    for i, (s, a) in enumerate(zip(seeds, al)):
        hb, hp = rt.vrf_prove(s, a)
        assert bytes(pi[i]) == hp, i
        assert bytes(beta[i]) == hb, i
        assert rt.vrf_beta(s, a) == hb
    assert rt.vrf_verify(rt.vrf_public_key(seeds[0]), al[0], bytes(pi[0])) == bytes(beta[0])


def test_outputs_only_job_and_device_queue(rt):
    from biscotti_amd.ops.vrf import DeviceVrfProver
    rng = np.random.default_rng(4)
    seeds = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(40)]
    alpha = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    job = rt.vrf_prove_batch_async(seeds, alpha, 4, None, True)
    full = rt.vrf_prove_batch(seeds, alpha, 4)
    assert job.betas() == [b for b, _ in full]
    prover = DeviceVrfProver("cuda", batch_rounds=2)
    st = torch.cuda.Stream()
    prover.submit(seeds[:20], alpha, st)
    assert prover.proofs == 0
    prover.submit(seeds[20:], alpha, st)       # second round: one launch for both
    assert prover.proofs == 40
    prover.submit(seeds[:5], alpha, st)
    prover.drain(st)
    assert prover.proofs == 45


# ------------------------------------------------------------------------------------------- edges
SENTINEL = 0xA5
SPARE = 16   # rows past n in pi, beta and scratch that a launch must leave alone


def _rows(a: np.ndarray):
    return [bytes(r) for r in a]


def _check(pi, beta, pairs):
    """Device rows against the reference, proof by proof."""
    assert len(pi) == len(pairs)
    for i, (s, a) in enumerate(pairs):
        rp, rb = V.expected(s, a)
        assert pi[i] == rp, i
        if beta is not None:
            assert beta[i] == rb, i


@pytest.fixture(scope="module")
def btab(rt):
    return torch.from_numpy(np.frombuffer(rt.vrf_base_table(), np.int32).copy()).to("cuda")


def _direct(btab, rows, key_idx, alphas, alpha_idx, alpha_len, n, beta=True, urgent=0):
    """One call of bsc_vrf_prove_p on key rows (96 bytes each) built by the test.  Returns (return value, pi rows,
    beta rows or None) after a sync, and checks that nothing past row n of pi, beta or scratch was written."""
    from biscotti_amd.native import hip
    from biscotti_amd.utils import streams as S
    # the kernel trusts its indices: keep every read in bounds (a launch also reads entry 0 of both index arrays)
    assert all(len(r) == 96 for r in rows)
    assert not 0 <= alpha_len <= 1024 or all(len(a) == alpha_len for a in alphas)
    assert len(key_idx) == len(alpha_idx) >= max(n, 1)
    assert 0 <= min(key_idx) and max(key_idx) < len(rows) and 0 <= min(alpha_idx) and max(alpha_idx) < len(alphas)
    dev = "cuda"
    m = max(n, 0) + SPARE
    keys = torch.from_numpy(np.frombuffer(b"".join(rows), np.int32).copy()).to(dev)
    al = torch.from_numpy(np.frombuffer(b"".join(alphas) + b"\x00", np.uint8).copy()).to(dev)
    kidx = torch.tensor(list(key_idx), dtype=torch.int32, device=dev)
    aidx = torch.tensor(list(alpha_idx), dtype=torch.int32, device=dev)
    pi = torch.full((m, 80), SENTINEL, dtype=torch.uint8, device=dev)
    bt = torch.full((m, 64), SENTINEL, dtype=torch.uint8, device=dev) if beta else None
    scratch = torch.full((m, 320 * 4), SENTINEL, dtype=torch.uint8, device=dev)
    ret = hip().bsc_vrf_prove_p(keys.data_ptr(), kidx.data_ptr(), al.data_ptr(), aidx.data_ptr(), alpha_len, n,
                                btab.data_ptr(), scratch.data_ptr(), pi.data_ptr(),
                                bt.data_ptr() if beta else None, urgent, S.raw())
    torch.cuda.synchronize()
    pi, scratch = pi.cpu().numpy(), scratch.cpu().numpy()
    k = max(n, 0) if ret == 0 else 0
    assert (pi[k:] == SENTINEL).all() and (scratch[k:] == SENTINEL).all()
    if beta:
        bt = bt.cpu().numpy()
        assert (bt[k:] == SENTINEL).all()
    return ret, _rows(pi[:k]), _rows(bt[:k]) if beta else None


def _prove_pairs(pairs):
    """(seed, alpha) pairs with alphas of one length through DeviceVrfProver.prove, outputs included."""
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda")
    pi, beta = prover.prove([s for s, _ in pairs], [a for _, a in pairs], beta=True)
    torch.cuda.synchronize()
    return _rows(pi.cpu().numpy()), _rows(beta.cpu().numpy())


def test_counters_mixed_in_one_workgroup():
    """First counters 0, 1, 11, 12, 13, 14, 15 and 17 in one workgroup of 16: the proofs that end in the first
    pass of 12 counters keep their H while lanes 1, 4, 6, 8, 11 and 13 go through the second pass."""
    pairs = V.inputs_counter_mix()
    assert len(pairs) == 16
    _check(*_prove_pairs(pairs), pairs)


def test_counters_all_in_the_second_pass():
    pairs = V.inputs_counter_high()
    assert len(pairs) == 16
    _check(*_prove_pairs(pairs), pairs)


def test_every_slot_publishes_h():
    """12 workgroups; lane 0 of workgroup g has first counter g, so every (wave, sub-lane) slot publishes H."""
    pairs = V.inputs_counter_slots()
    assert len(pairs) == 192
    _check(*_prove_pairs(pairs), pairs)


def test_crafted_scalars(rt, btab):
    """Key rows x || prefix || x*B with scalars at the edges of the signed radix-16 recoding and of the
    reduction mod L (test_vrf_edges.CRAFTED_X), two alphas each, through the direct call."""
    names = list(V.CRAFTED_X)
    keyrows = [V.crafted_row(V.CRAFTED_X[nm]) for nm in names]
    key_idx = [k for k in range(len(names)) for _ in V.CRAFTED_ALPHAS]
    alpha_idx = [(k + j) % 2 for k in range(len(names)) for j in range(len(V.CRAFTED_ALPHAS))]
    n = len(key_idx)
    ret, pi, beta = _direct(btab, [V.row_bytes(*r) for r in keyrows], key_idx, V.CRAFTED_ALPHAS, alpha_idx, 32, n)
    assert ret == 0
    for i in range(n):
        nm, row, alpha = names[key_idx[i]], keyrows[key_idx[i]], V.CRAFTED_ALPHAS[alpha_idx[i]]
        rp, rb, _ = E.prove(*row, alpha)
        assert pi[i] == rp, nm
        assert beta[i] == rb, nm
        if V.CRAFTED_X[nm] % E.L:
            assert rt.vrf_verify(row[2], alpha, pi[i]) == beta[i], nm
        else:
            assert pi[i][:32] == E.enc(E.IDENTITY), nm


@pytest.mark.parametrize("alpha_len", V.ALPHA_LENS)
def test_alpha_lengths(btab, alpha_len):
    """36 + alpha_len hashed bytes: in-block padding, its spill into a second block (112..127), the exact
    block, and two and more blocks; two alphas per launch, indexed 1 0 1 0 1, keys 2 0 1 2 0."""
    rows = [V.row_bytes(*E.key_from_seed(s)) for s in V.LEN_SEEDS]
    alphas = V.len_alphas(alpha_len)
    n = len(V.LEN_KEY_IDX)
    ret, pi, beta = _direct(btab, rows, V.LEN_KEY_IDX, alphas, V.LEN_ALPHA_IDX, alpha_len, n)
    assert ret == 0
    _check(pi, beta, [(V.LEN_SEEDS[k], alphas[a]) for k, a in zip(V.LEN_KEY_IDX, V.LEN_ALPHA_IDX)])


def test_rejected_arguments_write_nothing(btab):
    rows = [V.row_bytes(*E.key_from_seed(s)) for s in V.LEN_SEEDS]
    idx = [0, 1, 2, 0, 1]
    for alpha_len in (-1, 1025):
        ret, pi, _ = _direct(btab, rows, idx, [bytes(2048)], [0] * 5, alpha_len, 5)   # _direct checks the sentinels
        assert ret == -1 and pi == []
    for n in (0, -3):
        ret, pi, _ = _direct(btab, rows, idx, [bytes(32)], [0] * 5, 32, n)
        assert ret == 0 and pi == []


@pytest.mark.parametrize("n", V.BATCH_NS)
def test_batch_sizes_and_partial_workgroups(btab, n):
    """n around the 16 proofs of a workgroup: the lanes past n read row 0 and must write nothing (16 spare
    sentinel rows in pi, beta and scratch); pi does not depend on whether beta is asked for, nor on urgent."""
    pairs = V.inputs_batch()[:n]
    rows = [V.row_bytes(*E.key_from_seed(s)) for s in V.POOL_SEEDS[:n]]
    key_idx = list(range(n))
    alpha_idx = [i % 2 for i in range(n)]
    ret, pi, beta = _direct(btab, rows, key_idx, V.POOL_ALPHAS[:2], alpha_idx, 32, n)
    assert ret == 0
    _check(pi, beta, pairs)
    ret, pi_nobeta, none = _direct(btab, rows, key_idx, V.POOL_ALPHAS[:2], alpha_idx, 32, n, beta=False)
    assert ret == 0 and none is None and pi_nobeta == pi
    ret, pi_urgent, beta_urgent = _direct(btab, rows, key_idx, V.POOL_ALPHAS[:2], alpha_idx, 32, n, urgent=1)
    assert ret == 0 and pi_urgent == pi and beta_urgent == beta


# ---- the wrapper: the proofs of a flush are read from prover._inflight[-1] before drain, after a sync
def _submit_rounds(prover, rounds, st, as_rows=False):
    pairs = []
    for sl, a in rounds:
        seeds = V.POOL_SEEDS[sl]
        prover.submit(np.asarray(prover._rows(seeds), np.int32) if as_rows else seeds, V.POOL_ALPHAS[a], st)
        pairs += [(s, V.POOL_ALPHAS[a]) for s in seeds]
    return pairs


def _inflight_pi(prover, n):
    held = prover._inflight[-1][1]
    pi = held[0] if isinstance(held, tuple) else held   # one round holds (pi, scratch, upload), several hold pi
    torch.cuda.synchronize()
    assert pi.shape == (n, 80)
    return _rows(pi.cpu().numpy())


@pytest.mark.parametrize("urgent", [False, True])
def test_flush_of_one_round_packed_upload(urgent):
    """One queued round: rows, zero message indices and the message travel in one buffer."""
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda", batch_rounds=2)
    st = torch.cuda.Stream()
    pairs = _submit_rounds(prover, V.WRAP_ONE, st)
    assert prover.proofs == 0
    prover.flush(st, urgent=urgent)
    assert prover.proofs == len(pairs) == 21
    _check(_inflight_pi(prover, len(pairs)), None, pairs)
    prover.drain(st)
    assert prover._inflight == []


def test_flush_of_several_rounds_reuses_the_buffer():
    """Two and three queued rounds of different sizes and alphas (one launch each, the per-stream buffer), then
    a smaller batch on the same stream in the same buffer."""
    from biscotti_amd.ops.vrf import DeviceVrfProver
    st = torch.cuda.Stream()
    prover = DeviceVrfProver("cuda", batch_rounds=2)
    pairs = _submit_rounds(prover, V.WRAP_TWO, st)
    assert prover.proofs == len(pairs) == 37
    _check(_inflight_pi(prover, len(pairs)), None, pairs)
    prover.drain(st)
    prover = DeviceVrfProver("cuda", batch_rounds=3)
    pairs = _submit_rounds(prover, V.WRAP_THREE, st)
    assert prover.proofs == len(pairs) == 30
    _check(_inflight_pi(prover, len(pairs)), None, pairs)
    small = _submit_rounds(prover, V.WRAP_THREE_SMALL, st)
    assert prover.proofs == 30 + len(small) == 39
    assert prover._inflight[-1][1].data_ptr() == prover._inflight[-2][1].data_ptr()   # the same buffer
    _check(_inflight_pi(prover, len(small)), None, small)
    prover.drain(st)


def test_submit_of_key_rows():
    """submit given the int32 key rows (what the engine passes) instead of seeds."""
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda")
    prover._rows(V.POOL_SEEDS[:8])   # rows 0..7 taken, so the round's rows are not 0..n-1
    st = torch.cuda.Stream()
    pairs = _submit_rounds(prover, V.WRAP_ROWS, st, as_rows=True)
    assert prover.proofs == len(pairs) == 11
    _check(_inflight_pi(prover, len(pairs)), None, pairs)
    prover.drain(st)


def test_prove_repeats_interleaving_and_new_keys():
    """Repeated seeds and interleaved alphas in one prove; then a prove that adds keys after the key table was
    uploaded: the old rows and the new ones both prove correctly."""
    from biscotti_amd.ops.vrf import DeviceVrfProver
    prover = DeviceVrfProver("cuda")
    for plan in (V.PROVE_FIRST, V.PROVE_SECOND):
        pairs = [(V.POOL_SEEDS[s], V.POOL_ALPHAS[a]) for s, a in plan]
        keys_before = prover._keys_dev
        pi, beta = prover.prove([s for s, _ in pairs], [a for _, a in pairs], beta=True)
        assert prover._keys_dev is not keys_before   # new seeds: the key table was uploaded again
        torch.cuda.synchronize()
        _check(_rows(pi.cpu().numpy()), _rows(beta.cpu().numpy()), pairs)
    assert len(prover._keys) == 6
