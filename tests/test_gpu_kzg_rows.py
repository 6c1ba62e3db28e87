"""verifySecret per worker update on the device (K13, --kzg-audit shares): kzg.hip's row kernel (bsc_kzg_rlc_rows)
over the share MSM's unsummed output against the host oracle (kzg_rlc_host under the row's seed), the pairing
product accepting honest rows and rejecting exactly the tampered ones, skipped rows never read, and the engine's
per-worker audit naming the peer whose share was changed without touching the chain."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, POLY, N, SECRET = 21, 10, 5, 2
ALL = np.arange(T)
# two of three miners, their share slices in permuted order (parts {2: 0, 0: 2}, miner 0 listed first)
TWO = np.concatenate([14 + np.arange(7), np.arange(7)])
COLS = {"all21": ALL, "perm14": TWO}
_cache: dict = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def _rows(rt, d):
    """Device shares of N rows, unsummed, and every point of them as a host group element (computed once per d).
    Row 0: all-zero coefficients (every point at infinity); row 4: one nonzero coefficient, past chunk 0 when there
    is a second chunk; rows 1-3: random in +-10^6."""
    if d not in _cache:
        from biscotti_amd.ops import bn256 as B
        key = rt.CommitKey.generate(d, SECRET)
        eng = B.DeviceCommitEngine(key, POLY, T, b0=10)
        coeffs = np.random.default_rng(d).integers(-10**6, 10**6, size=(N, d), dtype=np.int64)
        coeffs[0] = 0
        coeffs[4] = 0
        coeffs[4, min(23, d - 1)] = -777
        pts, ys = eng.shares(torch.from_numpy(coeffs).cuda(), torch.arange(N, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert (ys.cpu().numpy() < 0).any() and (ys.cpu().numpy() > 0).any()
        g2 = rt.g2_generator()
        _cache[d] = {"key": key, "eng": eng, "pts": pts, "ys": ys, "g2": (g2, rt.g2_mul(g2, SECRET))}
    return _cache[d]


def _host_points(rt, pts):
    """pts [n, nch, T+1, 24] -> nested lists of marshalled points."""
    h = pts.cpu().numpy().view(np.uint32)
    return [[[rt.g1_from_device_jac(p) for p in ch] for ch in row] for row in h]


def _oracle(rt, c, P, ys_h, cols, seed, literal=False, rows=range(N)):
    """{row: (L1, A, L2)} from kzg_rlc_host under the row seeds."""
    from biscotti_amd.ops.bn256 import kzg_row_seed
    nch = len(P[0])
    bases = [rt.g1_generator()] if literal else [c["key"].point(POLY * k) for k in range(nch)]
    xs = [int(v) - 10 for v in cols]
    out = {}
    for i in rows:
        C = [P[i][k][T] for k in range(nch)]
        W = [P[i][k][int(j)] for k in range(nch) for j in cols]
        out[i] = tuple(rt.kzg_rlc_host(C, W, ys_h[i][:, cols].reshape(-1), xs, bases, kzg_row_seed(seed, i), 4))
    return out


def _triples(rt, out):
    h = out.cpu().numpy().view(np.uint32)
    return [tuple(rt.g1_from_device_jac(p) for p in row) for row in h]


def _is_inf(out, i):
    return bool((out[i, :, 16:] == 0).all())   # Jacobian infinity <=> z == 0


@pytest.mark.parametrize("d", [57, 10])
@pytest.mark.parametrize("cols", ["all21", "perm14"])
def test_rows_match_host_and_pairing_accepts(rt, d, cols):
    c, cols, seed = _rows(rt, d), COLS[cols], 0xC0FFEE1234
    eng, pts, ys = c["eng"], c["pts"], c["ys"]
    assert eng.nchunks == (6 if d == 57 else 1)
    out = eng.kzg_rlc_rows(pts, ys, _dev(cols), _dev(cols - 10), seed=seed)
    assert tuple(out.shape) == (N + 1, 3, 24) and out.dtype == torch.int32
    got = _triples(rt, out)
    P = c.setdefault("P", _host_points(rt, pts))
    want = _oracle(rt, c, P, ys.cpu().numpy(), cols, seed)
    tot = None
    for i in range(N):
        assert got[i] == want[i], f"row {i}"
        assert rt.kzg_check(*got[i], *c["g2"]), f"row {i}"
        tot = want[i] if tot is None else tuple(rt.g1_add(a, b) for a, b in zip(tot, want[i]))
    assert got[N] == tot
    assert rt.kzg_check(*got[N], *c["g2"])
    assert _is_inf(out, 0)   # the all-zero row: three infinities, accepted above
    # one share of one row the reference's way
    i, k, j = 2, eng.nchunks - 1, 3
    y = int(ys[i, k, int(cols[j])])
    assert rt.verify_secret(P[i][k][T], P[i][k][int(cols[j])], *c["g2"], int(cols[j]) - 10, y, c["key"].point(POLY * k))
    assert not rt.verify_secret(P[i][k][T], P[i][k][int(cols[j])], *c["g2"], int(cols[j]) - 10, y + 1,
                                c["key"].point(POLY * k))


def test_skipped_row_is_never_read(rt):
    c = _rows(rt, 57)
    eng, cols, seed = c["eng"], _dev(ALL), 77
    base = eng.kzg_rlc_rows(c["pts"], c["ys"], cols, _dev(ALL - 10), seed=seed)
    pts, ys = c["pts"].clone(), c["ys"].clone()
    pts[2].view(torch.uint8).fill_(0x7F)
    ys[2].view(torch.uint8).fill_(0x7F)
    alive = _dev(np.array([1, 1, 0, 1, 1]))
    out = eng.kzg_rlc_rows(pts, ys, cols, _dev(ALL - 10), alive=alive, seed=seed)
    assert _is_inf(out, 2)
    a, b = _triples(rt, base), _triples(rt, out)
    for i in (0, 1, 3, 4):
        assert a[i] == b[i], f"row {i}"
    P = c.setdefault("P", _host_points(rt, c["pts"]))
    want = _oracle(rt, c, P, c["ys"].cpu().numpy(), ALL, seed, rows=(0, 1, 3, 4))
    tot = None
    for i in (0, 1, 3, 4):
        tot = want[i] if tot is None else tuple(rt.g1_add(x, y) for x, y in zip(tot, want[i]))
    assert b[N] == tot and rt.kzg_check(*b[N], *c["g2"])
    # all flags set: the same as no flags
    ones = eng.kzg_rlc_rows(c["pts"], c["ys"], cols, _dev(ALL - 10), alive=_dev(np.ones(N)), seed=seed)
    assert _triples(rt, ones) == a


@pytest.mark.parametrize("cols", ["all21", "perm14"])
def test_tampered_rows_are_the_rejected_rows(rt, cols):
    c, cols = _rows(rt, 57), COLS[cols]
    eng = c["eng"]
    pts, ys = c["pts"].clone(), c["ys"].clone()
    s0, s1 = int(cols[5]), int(cols[6])
    pts[2, 1, s0] = c["pts"][2, 1, s1]     # one witness of row 2 swapped with its neighbour
    pts[2, 1, s1] = c["pts"][2, 1, s0]
    ys[1, 3, int(cols[4])] += 1            # one share value of row 1 off by one
    pts[3, 2, T] = c["pts"][3, 1, T]       # one chunk commitment of row 3 replaced
    out = eng.kzg_rlc_rows(pts, ys, _dev(cols), _dev(cols - 10), seed=99)
    got = _triples(rt, out)
    assert not rt.kzg_check(*got[N], *c["g2"])
    assert [i for i in range(N) if not rt.kzg_check(*got[i], *c["g2"])] == [1, 2, 3]
    h = out.cpu().numpy().view(np.uint32)
    assert not rt.kzg_check_device_async(h[N], *c["g2"]).result()
    assert rt.kzg_check_device_async(h[4], *c["g2"]).result()


def test_literal_form_holds_for_chunk_zero_only(rt):
    """y against G1 (the reference's formula) instead of PK[poly * k]: quirk Q9."""
    c = _rows(rt, 10)
    out = c["eng"].kzg_rlc_rows(c["pts"], c["ys"], _dev(ALL), _dev(ALL - 10), literal=True, seed=5)
    got = _triples(rt, out)
    assert all(rt.kzg_check(*t, *c["g2"]) for t in got)
    c = _rows(rt, 57)
    out = c["eng"].kzg_rlc_rows(c["pts"], c["ys"], _dev(ALL), _dev(ALL - 10), literal=True, seed=5)
    got = _triples(rt, out)
    P = c.setdefault("P", _host_points(rt, c["pts"]))
    want = _oracle(rt, c, P, c["ys"].cpu().numpy(), ALL, 5, literal=True)
    assert all(got[i] == want[i] for i in range(N))
    # row 0 has no coefficients at all, row 4 its only one in chunk 2, rows 1-3 in every chunk
    assert [rt.kzg_check(*got[i], *c["g2"]) for i in range(N)] == [True, False, False, False, False]


def test_no_rows_and_bad_arguments(rt):
    c = _rows(rt, 57)
    eng = c["eng"]
    out = eng.kzg_rlc_rows(c["pts"][:0], c["ys"][:0], _dev(ALL), _dev(ALL - 10), seed=1)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 3, 24) and _is_inf(out, 0)
    out = eng.kzg_rlc_rows(c["pts"], c["ys"], _dev(ALL[:0]), _dev(ALL[:0]), seed=1)
    assert tuple(out.shape) == (N + 1, 3, 24) and all(_is_inf(out, i) for i in range(N + 1))
    from biscotti_amd.native import hip
    p = c["pts"].data_ptr()
    assert hip().bsc_kzg_rlc_rows(p, p, None, p, p, 1, 6, T, 33, p, 10, 0, p, p, None) == -1   # npts > 32
    assert hip().bsc_kzg_rlc_rows(p, p, None, p, p, 1, 6, T, 21, p, -1, 0, p, p, None) == -1   # negative stride
    assert hip().bsc_kzg_rlc_rows(p, p, None, None, p, 1, 6, T, 21, p, 10, 0, p, p, None) == -1   # no columns
    assert hip().bsc_kzg_rlc_rows(p, p, None, p, p, 0, 6, T, 21, p, 10, 0, p, p, None) == 0


# ---------------------------------------------------------------------------------------------- the engine
ROUNDS = 6


def _engine(mode):
    from biscotti_amd.parallel.comm import Comm
    from biscotti_amd.protocol.config import RunConfig
    from biscotti_amd.protocol.engine import BiscottiEngine

    cfg = RunConfig(num_nodes=20, seed=3, deterministic_time=True, kzg_audit=mode)
    return BiscottiEngine(cfg, Comm(device=torch.device("cuda", 0)))


def _hashes(eng):
    return [bytes(eng.fsm.chain.block(i).hash) for i in range(len(eng.fsm.chain))]


@pytest.fixture(scope="module")
def honest():
    """The same six rounds without the audit and with it (narrow tables: the chain does not depend on them)."""
    old = os.environ.get("BSC_TABLE_B0")
    os.environ["BSC_TABLE_B0"] = "10"
    out = {}
    try:
        for mode in ("off", "shares"):
            eng = _engine(mode)
            try:
                res = [eng.run_round() for _ in range(ROUNDS)]
                eng.drain()
                out[mode] = {"res": res, "hashes": _hashes(eng), "stats": dict(eng.stats),
                             "verify": eng.fsm.chain.verify()[0]}
            finally:
                eng.close()
        yield out
    finally:
        if old is None:
            os.environ.pop("BSC_TABLE_B0", None)
        else:
            os.environ["BSC_TABLE_B0"] = old


def test_engine_audits_every_update_and_keeps_the_chain(honest):
    run = honest["shares"]
    blocks = [r for r in run["res"] if r is not None and not r.empty]
    assert len(blocks) >= 4
    st = run["stats"]
    assert st["kzg_checks"] == len(blocks) and st["kzg_failures"] == 0
    assert st["kzg_share_failures"] == 0
    assert st["kzg_share_checks"] == sum(len(r.node_list) for r in blocks)
    assert run["verify"]
    assert run["hashes"] == honest["off"]["hashes"]


def test_engine_blames_the_peer_whose_share_was_changed(honest, monkeypatch):
    """One share value of one audited row, changed by one in a clone handed to the row kernel in one iteration:
    that (iteration, peer) is reported and counted, nothing else is, and the chain is the honest run's."""
    monkeypatch.setenv("BSC_TABLE_B0", "10")
    blocks = [r for r in honest["shares"]["res"] if r is not None and not r.empty]
    target = blocks[2].iteration
    eng = _engine("shares")
    try:
        launch, hit = eng._kzg_rows_launch, []

        def tampered(pts, ys, alive, cols, xs, rows, it):
            if it != target:
                return launch(pts, ys, alive, cols, xs, rows, it)
            r = int(alive.cpu().numpy().nonzero()[0][0])
            ys = ys.clone()
            ys[r, 0, int(cols[0])] += 1
            e = launch(pts, ys, alive, cols, xs, rows, it)
            hit.append((e, rows[r]))
            return e

        eng._kzg_rows_launch = tampered
        for _ in range(ROUNDS):
            eng.run_round()
        eng.drain()
        adopted = [w for e, w in hit if "rows_done" in e]   # (an aggregate can be queued twice; one is adopted)
        assert len(adopted) == 1 and adopted[0] in blocks[2].node_list
        assert eng.kzg_share_blame == [(target, adopted[0])]
        st = eng.stats
        assert st["kzg_share_failures"] == 1 and st["kzg_failures"] == 1
        assert st["kzg_checks"] == len(blocks)
        assert st["kzg_share_checks"] == honest["shares"]["stats"]["kzg_share_checks"]
        assert eng.fsm.chain.verify()[0]
        assert _hashes(eng) == honest["off"]["hashes"]
    finally:
        eng.close()
