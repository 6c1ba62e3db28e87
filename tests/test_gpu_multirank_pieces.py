"""The multi-rank round's device pieces, each against an exact reference, in ONE process on one GPU.

The whole-engine runs of test_gpu_multirank.py spawn 2 to 8 processes and compare chain hashes; these tests call
the pieces directly -- the verification row's pack / unpack (kernels/gather.hip), the split Gram written into the
packed row, the partial sums with their clock word, the strided recovery with its pinned mirrors, the two halves of
the aggregation around the gather the caller issues, and the emulated collectives -- with every rank simulated in
turn: each rank's half into its own row, the rows copied together, the second half.  Everything is data movement or
exact integer / group arithmetic, so the references are numpy models and Python integers written here.

Shapes: a commitment key with d = 85, poly = 10, T = 21, so nch = 9 -- the recovery's second block holds one chunk
(8 chunks per block) and the last chunk is half full (d < nch * poly).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from biscotti_amd.native import hip
from biscotti_amd.ops import bn256 as B
from biscotti_amd.ops import ml as K
from biscotti_amd.ops.gather import VerifyGather
from biscotti_amd.utils import streams as S

pytestmark = pytest.mark.gpu

D, POLY, T = 85, 10, 21
NCH = 9
QS = 1e4
ALL21 = list(range(21))
OUTER14 = list(range(0, 7)) + list(range(14, 21))   # two of three miners: x in -10..-4 and 4..10


def _bytes(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same_bytes(got, want, what=""):
    np.testing.assert_array_equal(_bytes(got), _bytes(want), err_msg=what)


def _sentinel(nbytes: int, pinned: bool = False, value: int = 0x5A) -> torch.Tensor:
    if pinned:
        t = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        t.fill_(value)
        return t
    return torch.full((nbytes,), value, dtype=torch.uint8, device="cuda")


def _comm(world: int, rank: int = 0):
    return SimpleNamespace(world=world, rank=rank, emulating=True, backend="none")


# ------------------------------------------------------------------------------------------------------------
# a. the verification row: [ Gram slot: chunk x 256 f64 | commitments: maxlocal x pw u32 | noiser ids: maxlocal x
#    nn i32 | noiser weights: maxlocal x nn f32 ], padded to 16 bytes (the header comment of kernels/gather.hip)
def _row_model(chunk, maxlocal, pw, nn):
    gram_bytes = chunk * 256 * 8
    commit_off = gram_bytes
    nz_off = commit_off + 4 * maxlocal * pw
    sc_off = nz_off + 4 * maxlocal * nn
    end = sc_off + 4 * maxlocal * nn
    return gram_bytes, commit_off, nz_off, sc_off, end, -(-end // 16) * 16


SPECIAL_WEIGHTS = np.array([-0.0, 1e-45, np.finfo(np.float32).max], np.float32)   # -0, a denormal, the largest finite


class _VgRows:
    """Every rank's inputs of one case and the numpy model of the gathered buffer they give."""

    def __init__(self, world, maxlocal, nn, pw, chunk, seed, src_rows=None, ranks=None):
        rng = np.random.default_rng(seed)
        self.shape = (world, maxlocal, nn, pw, chunk)
        self.gram_bytes, self.commit_off, self.nz_off, self.sc_off, self.end, self.row_bytes = \
            _row_model(chunk, maxlocal, pw, nn)
        self.model = np.full((world, self.row_bytes), 0xA5, np.uint8)
        self.slots = rng.standard_normal((world, chunk, 256))
        self.model[:, :self.gram_bytes] = self.slots.reshape(world, -1).view(np.uint8)
        self.ranks = []
        nsrc = maxlocal + 2
        for r in (range(world) if ranks is None else ranks):
            commits = rng.integers(0, 2 ** 32, size=(nsrc, pw), dtype=np.uint64).astype(np.uint32)
            src = np.asarray(src_rows[r], np.int32) if src_rows is not None else \
                rng.integers(-1, nsrc, size=maxlocal).astype(np.int32)
            nz = rng.integers(-2 ** 31, 2 ** 31, size=(maxlocal, nn)).astype(np.int32)
            sc = rng.standard_normal((maxlocal, nn)).astype(np.float32)
            flat = sc.reshape(-1)
            for i, v in enumerate(SPECIAL_WEIGHTS):
                if flat.size:
                    flat[(i + r) % flat.size] = v
            packed = np.where(src[:, None] >= 0, commits[np.maximum(src, 0)], 0).astype(np.uint32)
            self.model[r, self.commit_off:self.nz_off] = _bytes(packed)
            self.model[r, self.nz_off:self.sc_off] = _bytes(nz)
            self.model[r, self.sc_off:self.end] = _bytes(sc)
            self.ranks.append(SimpleNamespace(commits=commits, src=src, nz=nz, sc=sc, packed=packed))

    def start(self) -> torch.Tensor:
        """The buffer before any pack: the sentinel with every rank's Gram slot at its row's head."""
        first = np.full_like(self.model, 0xA5)
        first[:, :self.gram_bytes] = self.model[:, :self.gram_bytes]
        return torch.from_numpy(first).cuda()

    def expect_unpacked(self, npairs, wrow):
        world, maxlocal, nn, pw, chunk = self.shape
        gram = np.stack([self.slots[p // chunk, p % chunk] for p in range(npairs)]) if npairs else np.zeros((0, 256))
        nz = np.concatenate([q.nz for q in self.ranks])
        sc = np.concatenate([q.sc for q in self.ranks])
        rows = [self.ranks[f // maxlocal].packed[f % maxlocal] for f in wrow]
        commits = np.stack(rows) if rows else np.zeros((0, pw), np.uint32)
        return gram, nz, sc, commits


def _unpack_and_compare(buf, m: _VgRows, npairs, wrow):
    world, maxlocal, nn, pw, chunk = m.shape
    nw = len(wrow)
    gram = _sentinel((npairs + 1) * 2048)
    nzo, sco = (_sentinel((world * maxlocal * nn + 4) * 4) for _ in range(2))
    host = _sentinel((nw + 1) * pw * 4, pinned=True)
    wr = np.ascontiguousarray(wrow if nw else [0], np.int32)
    assert hip().bsc_vg_unpack(buf.data_ptr(), m.row_bytes, chunk, npairs, m.commit_off, m.nz_off, m.sc_off, maxlocal,
                               pw, nn, world, wr.ctypes.data, nw, gram.data_ptr(), nzo.data_ptr(), sco.data_ptr(),
                               host.data_ptr(), S.raw()) == 0
    torch.cuda.synchronize()
    e_gram, e_nz, e_sc, e_commits = m.expect_unpacked(npairs, wrow)
    guard = lambda n: np.full(n, 0x5A, np.uint8)
    _same_bytes(gram, np.concatenate([_bytes(e_gram), guard(2048)]), "tiled Gram")
    _same_bytes(nzo, np.concatenate([_bytes(e_nz), guard(16)]), "flat noiser ids")
    _same_bytes(sco, np.concatenate([_bytes(e_sc), guard(16)]), "flat noiser weights (bit patterns)")
    _same_bytes(host.numpy(), np.concatenate([_bytes(e_commits), guard(pw * 4)]), "pinned commitment rows")


VG_CASES = {
    "one": dict(world=1, maxlocal=1, nn=1, pw=24, chunk=1, npairs=1, wrow=[0], src_rows=[[1]]),
    # npairs no multiple of chunk (the last rank's slot half used); -1 sources, a permutation, a repeated source
    # row; worker rows out of rank order, the last flat row among them
    "three": dict(world=3, maxlocal=5, nn=2, pw=24, chunk=4, npairs=10, wrow=[14, 3, 7, 0, 11, 5, 9],
                  src_rows=[[2, -1, 0, 1, -1], [4, 3, 2, 1, 0], [6, 6, -1, 0, 6]]),
    # both argument-block limits at once: maxlocal = 128 slots, maxlocal * nn = 256 noiser entries
    "limits": dict(world=4, maxlocal=128, nn=2, pw=24, chunk=2, npairs=7,
                   wrow=[511, 0, 128, 127] + list(range(300, 336))),
    "no-noisers": dict(world=2, maxlocal=3, nn=0, pw=24, chunk=1, npairs=2, wrow=[5, 0]),
    "no-workers": dict(world=3, maxlocal=5, nn=2, pw=24, chunk=4, npairs=10, wrow=[]),
}


@pytest.mark.parametrize("case", list(VG_CASES))
def test_verification_row_pack_unpack_every_rank(case):
    """bsc_vg_pack once per simulated rank into its row of one [world, row_bytes] buffer, bsc_vg_unpack once: the
    packed buffer (the bytes the pack must leave alone included: the Gram slot, the padding), the tiled Gram, the
    flat ids / weights and the pinned commitment rows equal the numpy model of the layout, byte for byte."""
    c = dict(VG_CASES[case])
    world, maxlocal, nn, pw, chunk, npairs, wrow = (c[k] for k in ("world", "maxlocal", "nn", "pw", "chunk", "npairs",
                                                                  "wrow"))
    assert case != "limits" or (len(wrow) == 40 and maxlocal * nn == 256)
    m = _VgRows(world, maxlocal, nn, pw, chunk, seed=len(case), src_rows=c.get("src_rows"))
    vg = VerifyGather(_comm(world), maxlocal, pw, nn, chunk, npairs, max(1, len(wrow)), "cuda")
    assert (vg.gram_bytes, vg.commit_off, vg.nz_off, vg.sc_off, vg.row_bytes) == \
        (m.gram_bytes, m.commit_off, m.nz_off, m.sc_off, m.row_bytes)
    buf = m.start()
    keep = []
    for r, q in enumerate(m.ranks):
        cd = torch.from_numpy(q.commits.view(np.int32)).cuda()
        keep.append(cd)
        assert hip().bsc_vg_pack(buf.data_ptr() + r * m.row_bytes, m.commit_off, m.nz_off, m.sc_off, cd.data_ptr(),
                                 maxlocal, pw, q.src.ctypes.data, q.nz.ctypes.data, q.sc.ctypes.data, maxlocal * nn,
                                 S.raw()) == 0
    torch.cuda.synchronize()
    _same_bytes(buf, m.model, "the packed rows")
    _unpack_and_compare(buf, m, npairs, wrow)


# ------------------------------------------------------------------------------------------------------------
# b. the split Gram written into the packed row
def _own_pairs(U, rank, world):
    tiles = (U + 15) // 16
    npairs = tiles * (tiles + 1) // 2
    chunk = -(-npairs // world)
    p0 = min(npairs, rank * chunk)
    return p0, min(npairs, p0 + chunk), chunk, npairs, tiles


def _dense_from_tiles(tiles_t, U):
    """[U, U] out of the tiled upper triangle: tile pairs (ti <= tj) row-major, entry [16 a + b] = G[16 ti + a][16 tj + b]"""
    nt = (U + 15) // 16
    G = np.zeros((nt * 16, nt * 16))
    t = tiles_t.cpu().numpy()
    k = 0
    for ti in range(nt):
        for tj in range(ti, nt):
            G[ti * 16:ti * 16 + 16, tj * 16:tj * 16 + 16] = t[k].reshape(16, 16)
            G[tj * 16:tj * 16 + 16, ti * 16:ti * 16 + 16] = t[k].reshape(16, 16).T
            k += 1
    assert not G[U:].any() and not G[:, U:].any()   # rows past U are zero operands
    return G[:U, :U]


def _split_gram_into_rows(X, T_rows, world, nn=None, kchunk=128):
    U = X.shape[0] + T_rows.shape[0]
    ref = K.gram_stacked_async(X, T_rows, kchunk=kchunk)["gram"]
    _, _, chunk, npairs, _ = _own_pairs(U, 0, world)
    vg = VerifyGather(_comm(world), 2, 24, 1, chunk, npairs, 1, "cuda")
    vg.recv[0].fill_(0xA5)
    keep = []
    for r in range(world):
        vg.comm = _comm(world, r)
        keep.append(K.gram_stacked_async(X, T_rows, kchunk=kchunk, split=(r, world), out=vg.gram_out(0), nn=nn))
    got = torch.full((npairs, 256), -1.0, dtype=torch.float64, device="cuda")
    assert hip().bsc_vg_unpack(vg.recv[0].data_ptr(), vg.row_bytes, chunk, npairs, vg.commit_off, vg.nz_off, vg.sc_off,
                               2, 24, 1, world, np.zeros(1, np.int32).ctypes.data, 0, got.data_ptr(), vg.nz.data_ptr(),
                               vg.sc.data_ptr(), vg.host[0].data_ptr(), S.raw()) == 0
    torch.cuda.synchronize()
    assert tuple(ref.shape) == (npairs, 256)
    assert torch.equal(got, ref), (world, (got - ref).abs().max().item())
    rows = vg.recv[0].cpu().numpy()
    for r in range(world):
        p0, p1, _, _, _ = _own_pairs(U, r, world)
        assert (rows[r, (p1 - p0) * 2048:] == 0xA5).all(), (world, r)   # nothing past the rank's own pairs
    return got


@pytest.fixture(scope="module")
def noise9():
    nr = K.NoiseRows(9, 300, 11, "cuda")
    return nr, nr.gram_table(kchunk=128)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("table", [False, True], ids=["computed", "table"])
@pytest.mark.parametrize("U1", [23, 16])
def test_split_gram_into_the_packed_row(noise9, U1, table, world):
    """Every rank's tile pairs of the [deltas; noise rows] Gram (U = 32 or 25: 3 pairs; D = 300 in K pieces of 128,
    the last one ragged) written by the kernel into its slot of the receive buffer, then unpacked: bit-identical to
    the unsplit Gram, equal to the fp64 product, nothing written past a rank's own pairs.  At 4 ranks rank 3 owns
    no pair; at 2 ranks rank 1's slot is half used.  With the table, U1 = 16 makes pair (1, 1) noise rows only (the
    copied tile); at U1 = 23 every tile holds a delta row, so the table is bound and nothing is copied."""
    nr, tab = noise9
    it = 7
    g = torch.Generator().manual_seed(U1 + world)
    X = (0.01 * torch.randn((U1, 300), generator=g)).float().cuda()
    got = _split_gram_into_rows(X, nr.rows(it), world, nn=tab[it] if table else None)
    rows = torch.cat([X, nr.rows(it)]).double().cpu()
    want = (rows @ rows.T).numpy()
    np.testing.assert_allclose(_dense_from_tiles(got, U1 + 9), want, rtol=1e-12, atol=1e-9)


def test_split_gram_one_pair_two_ranks():
    """U1 = 16 delta rows and no noise row: one tile pair, so rank 1 of 2 launches nothing."""
    X = (0.01 * torch.randn((16, 300), generator=torch.Generator().manual_seed(3))).float().cuda()
    none = torch.empty((0, 300), dtype=torch.float32, device="cuda")
    assert _own_pairs(16, 1, 2)[:2] == (1, 1)
    got = _split_gram_into_rows(X, none, 2)
    np.testing.assert_allclose(_dense_from_tiles(got, 16), (X.double() @ X.double().T).cpu().numpy(), rtol=1e-12,
                               atol=1e-9)


# ------------------------------------------------------------------------------------------------------------
# c. the partial sums with the clock word behind them
GUARD = -0x0123456789ABCDEF


@pytest.mark.parametrize("C", [1, 255, 256, NCH * T])
def test_sum_rows_i64_tail(C):
    """out[c] = the kept rows' int64 sum for c < C, out[C] = tail, out[C + 1] untouched: C + 1 ends one past a
    block (255), one into the next (256), and at the round's own 9 x 21."""
    R = 5
    rng = np.random.default_rng(C)
    lim = 2 ** 60 // R
    ys = rng.integers(-lim, lim, size=(R, C), dtype=np.int64, endpoint=True)
    ys[0, 0], ys[R - 1, C - 1] = lim, -lim
    ys_t = torch.from_numpy(ys).cuda()
    masks = {"none": None, "mixed": np.array([1, 0, 1, 1, 0], np.int32), "zero": np.zeros(R, np.int32)}
    for name, mask in masks.items():
        for tail in (0, -1, 2 ** 63 - 1):
            out = torch.full((C + 2,), GUARD, dtype=torch.int64, device="cuda")
            mt = torch.from_numpy(mask).cuda() if mask is not None else None
            assert hip().bsc_sum_rows_i64_tail(ys_t.data_ptr(), R, C, mt.data_ptr() if mt is not None else None,
                                               out.data_ptr(), tail, S.raw()) == 0
            want = (ys if mask is None else ys[mask.astype(bool)]).sum(0, dtype=np.int64)
            np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate([want, [tail, GUARD]]), err_msg=name)
    # no local rows: zeros and the clock, from null pointers
    out = torch.full((C + 2,), GUARD, dtype=torch.int64, device="cuda")
    assert hip().bsc_sum_rows_i64_tail(None, 0, C, None, out.data_ptr(), -77, S.raw()) == 0
    np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate([np.zeros(C, np.int64), [-77, GUARD]]))


# ------------------------------------------------------------------------------------------------------------
# d. the recovery over strided rows, with the clocks and the pinned mirrors
def _layout(cols):
    xs = np.asarray(cols) - 10
    w = K.recovery_weights(xs.tolist(), POLY)
    return SimpleNamespace(cols=list(cols), xs=xs, w=w, npts=len(cols),
                           ycols=torch.tensor(cols, dtype=torch.int32).cuda(),
                           xs_t=torch.from_numpy(xs.astype(np.int32)).cuda(),
                           A=torch.from_numpy(w["A"].reshape(-1)).cuda(),
                           basis=torch.tensor(w["basis"], dtype=torch.int32).cuda())


XPOW = np.array([[x ** j for x in range(-10, 11)] for j in range(POLY)], dtype=object)   # [poly][21], Python integers
SHARE_GROWTH = sum(10 ** j for j in range(POLY))   # |share| <= max|coefficient| * sum_j 10^j  (|x| <= 10)


def _int_shares(per):
    """[..., nch, poly] Python-integer coefficients -> [..., nch, 21] shares at x = -10..10."""
    return np.dot(per.astype(object), XPOW)


def _recover_strided(L, rows64, world, rstride, lead, W):
    """bsc_recover_w_clock on rows64 (int64 [world * rstride] on the device), sums at word `lead` of every row."""
    o = SimpleNamespace(
        W_new=torch.full((D + 4,), -7.25, dtype=torch.float64, device="cuda"),
        coeffs=torch.full((NCH, POLY), GUARD, dtype=torch.int64, device="cuda"),
        status=torch.full((NCH,), -3, dtype=torch.int32, device="cuda"),
        agg=torch.full((NCH, L.npts), GUARD, dtype=torch.int64, device="cuda"),
        h_W=torch.full((D + 4,), -7.25, dtype=torch.float64).pin_memory(),
        h_status=torch.full((NCH,), -3, dtype=torch.int32).pin_memory(),
        h_clock=torch.full((world + 1,), GUARD, dtype=torch.int64).pin_memory())
    w = L.w
    assert hip().bsc_recover_w_clock(rows64.data_ptr() + 8 * lead, world, rstride, NCH, T, None, L.ycols.data_ptr(),
                                     L.xs_t.data_ptr(), L.npts, L.A.data_ptr(), L.basis.data_ptr(), POLY, w["shift"],
                                     w["inv_lo"], w["inv_hi"], D, W.data_ptr(), QS, o.W_new.data_ptr(),
                                     o.coeffs.data_ptr(), o.status.data_ptr(), o.agg.data_ptr(), o.h_W.data_ptr(),
                                     o.h_status.data_ptr(), o.h_clock.data_ptr(), S.raw()) == 0
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("world", [1, 4])
@pytest.mark.parametrize("cols", [ALL21, OUTER14], ids=["all21", "outer14"])
@pytest.mark.parametrize("lead", [0, 12 * NCH], ids=["front", "behind-cs"])
@pytest.mark.parametrize("big", [False, True], ids=["3e6", "2^62"])
def test_strided_recovery_with_clocks(world, cols, lead, big):
    """k_recover_w over the ranks' rows inside a gathered buffer: rstride = row_bytes / 8 (300 words for 9 x 21 sums),
    each rank's sums at the row's front -- or, as the aggregation passes them, behind the 96 nch bytes of its
    commitment sums -- its clock right after them, garbage everywhere else; no mask; pinned mirrors.

    Magnitudes: per-rank coefficients up to 3 * 10^6, and up to M = (2^62 - 1) // (world * sum_j 10^j): a share is at
    most max|c| * sum_{j < 10} 10^j, so every share summed over the ranks stays below 2^62 -- checked on the
    Python-integer shares below, with coefficient rows that reach the bound at x = 10 and at x = -10."""
    rng = np.random.default_rng(world * 100 + len(cols) + lead)
    L = _layout(cols)
    rstride = hip().bsc_round_row_bytes(NCH, T) // 8
    assert rstride == 300 and lead + NCH * T + 1 <= rstride
    M = (2 ** 62 - 1) // (world * SHARE_GROWTH) if big else 3 * 10 ** 6
    per = rng.integers(-M, M, size=(world, NCH, POLY), dtype=np.int64, endpoint=True)
    per[:, 0, :] = M
    per[:, 1, :] = M * (-1) ** np.arange(POLY)
    per[:, 2, :] = -M
    shares = _int_shares(per)                                    # [world, nch, 21], Python integers
    tot_sh = shares.sum(0)
    assert max(abs(int(v)) for v in tot_sh.reshape(-1)) < 2 ** 62
    assert not big or max(abs(int(v)) for v in tot_sh.reshape(-1)) > 2 ** 62 - world * SHARE_GROWTH
    total = per.astype(object).sum(0)                            # [nch, poly]
    clocks = [1700000000123456789, -5, 0, 2 ** 63 - 1][:world]
    buf = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(world, rstride), dtype=np.int64, endpoint=True)
    buf[:, lead:lead + NCH * T] = shares.astype(np.int64).reshape(world, -1)
    buf[:, lead + NCH * T] = clocks
    W = torch.from_numpy(rng.standard_normal(D)).cuda()
    Wn = W.cpu().numpy()

    def expect(tot):
        return Wn + tot.reshape(-1)[:D].astype(np.float64) / QS

    o = _recover_strided(L, torch.from_numpy(buf).cuda().view(-1), world, rstride, lead, W)
    tot64 = total.astype(np.int64)
    np.testing.assert_array_equal(o.coeffs.cpu().numpy(), tot64)
    np.testing.assert_array_equal(o.agg.cpu().numpy(), tot_sh.astype(np.int64)[:, cols])
    assert o.status.cpu().tolist() == [1] * NCH and o.h_status.tolist() == [1] * NCH
    assert o.h_clock.tolist() == clocks + [GUARD]
    got_W = o.W_new.cpu().numpy()
    assert (got_W[D:] == -7.25).all() and (o.h_W.numpy()[D:] == -7.25).all()   # idx >= d is never written
    _same_bytes(o.h_W.numpy(), got_W, "pinned model mirror")
    np.testing.assert_allclose(got_W[:D], expect(tot64))

    # one flipped share word of one rank: exactly its chunk fails, in either block
    for k in (3, NCH - 1):
        bad = buf.copy()
        bad[world - 1, lead + k * T + cols[3]] ^= 1
        o = _recover_strided(L, torch.from_numpy(bad).cuda().view(-1), world, rstride, lead, W)
        want_st = [int(c != k) for c in range(NCH)]
        want_c = tot64.copy()
        want_c[k] = 0
        assert o.status.cpu().tolist() == want_st and o.h_status.tolist() == want_st
        np.testing.assert_array_equal(o.coeffs.cpu().numpy(), want_c)
        got_W = o.W_new.cpu().numpy()
        np.testing.assert_array_equal(got_W[k * POLY:min(D, (k + 1) * POLY)], Wn[k * POLY:min(D, (k + 1) * POLY)])
        np.testing.assert_allclose(got_W[:D], expect(want_c))
        _same_bytes(o.h_W.numpy(), got_W, "pinned model mirror")
        assert o.h_clock.tolist() == clocks + [GUARD]


# ------------------------------------------------------------------------------------------------------------
# e / f. the aggregation's halves and the emulated collectives
@pytest.fixture(scope="module")
def eng(rt):
    return B.DeviceCommitEngine(rt.CommitKey.generate(D, 3), POLY, T, b0=10)


@pytest.fixture(scope="module")
def shares7(eng):
    """Seven quantised rows, their shares (pts [7, nch, T + 1, 24], ys [7, nch, T]) and their Python-integer form."""
    q = np.random.default_rng(17).integers(-9000, 9000, size=(7, D), dtype=np.int64)
    pts, ys = eng.shares(torch.from_numpy(q).cuda(), torch.arange(7, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return q, pts, ys


class _Ctx:
    """One NativeSecAgg on three fresh streams with the two-miner layout registered (no task bound: the pre-step
    stays out through pre_it = -1)."""

    def __init__(self, eng):
        self.main, self.side, self.bg, self.upload = (torch.cuda.Stream() for _ in range(4))
        self.na = B.NativeSecAgg(eng, self.main, self.side, self.bg, QS)
        L = self.L = _layout(OUTER14)
        base = np.arange(NCH) * (T + 1)
        self.ccols = torch.from_numpy((base + T).astype(np.int32)).cuda()
        wc = (base[:, None] + np.asarray(L.cols)[None, :]).reshape(-1)
        self.wcols = torch.from_numpy(wc.astype(np.int32)).cuda()
        self.lid = self.na.add_layout(self.ccols, self.wcols, L.ycols, L.xs_t, L.w, L.A, L.basis)
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        self.na.close()


def _handle(pts, ys, mask):
    """What the round's calls read of a speculative MSM's handle; the flags are already set (node = None)."""
    n = pts.shape[0]
    h = SimpleNamespace(alive=torch.tensor(mask, dtype=torch.int32, device="cuda"), rows=list(range(n)),
                        rows_t=torch.arange(n, dtype=torch.int32, device="cuda"), pts=pts.contiguous(),
                        ys=ys.contiguous(), ev=torch.cuda.Event())
    torch.cuda.synchronize()
    h.ev.record()
    return h


def _results(c: _Ctx, W_new, clocks=False):
    """Everything a round reads back of one aggregation (host waits through the native read-backs first)."""
    na = c.na
    rb = na.readback(clocks=clocks)()
    ok = na.audit(queue=False)().copy()
    h_status, h_W = rb[0].copy(), rb[1].copy()
    torch.cuda.synchronize()
    r = SimpleNamespace(status=na.status.cpu().numpy(), coeffs=na.coeffs.cpu().numpy(), W_new=W_new.cpu().numpy(),
                        cs=B.marshal(na.cs).cpu().numpy(), ok=ok, h_status=h_status, h_W=h_W,
                        clock=rb[2].copy() if clocks else None)
    np.testing.assert_array_equal(r.h_status, r.status)
    _same_bytes(r.h_W, r.W_new, "pinned model mirror")
    return r


def _coeff_total(q, mask):
    tot = np.zeros(NCH * POLY, dtype=object)
    tot[:D] = q[np.asarray(mask, bool)].astype(object).sum(0) if any(mask) else 0
    return tot.reshape(NCH, POLY).astype(np.int64)


SPLIT = [(0, 4), (4, 7), (7, 7)]              # 7 rows over 3 ranks: 4 / 3 / none
CLOCKS = [1700000000123456789, -5, 77]


@pytest.fixture(scope="module")
def two_ctx(eng):
    multi, single = _Ctx(eng), _Ctx(eng)
    multi.na.gather_buffers(3)
    state = SimpleNamespace(multi=multi, single=single,
                            W=torch.from_numpy(np.random.default_rng(2).standard_normal(D)).cuda())
    yield state
    multi.close()
    single.close()


def _three_ranks_then_one(state, pts, ys, mask):
    """The 7 rows through select_partials per simulated rank + after_gather, and through after_select on the second
    context; returns (multi-rank results, one-rank results, the model the round started from)."""
    m, s, W = state.multi, state.single, state.W
    na = m.na
    keep = []   # the handles' tensors stay referenced until the streams that read them are done
    for r, (a, b) in enumerate(SPLIT):
        sp = _handle(pts[a:b], ys[a:b], mask[a:b]) if b > a else None
        keep.append(sp)
        na.select_partials(None, None, sp, -1, m.upload, m.lid, CLOCKS[r], 1)
        with torch.cuda.stream(m.main):
            na.recv[r].copy_(na.send)       # the gather: this rank's row into its slot, on the main stream
    W_new, pre = na.after_gather(m.lid, W, 1, -1)
    assert pre == -1
    # the recovered model lands in a ring slot that is not the one holding W
    assert W_new.data_ptr() != W.data_ptr() and any(W_new is t for t in na.W_ring)
    got = _results(m, W_new, clocks=True)
    W1 = W.clone()
    torch.cuda.synchronize()
    keep.append(_handle(pts, ys, mask))
    W_one, pre1 = s.na.after_select(None, None, keep[-1], -1, s.upload, s.lid, W1, 1, -1)
    assert pre1 is None
    one = _results(s, W_one)
    del keep
    W0 = W.cpu().numpy()
    state.W = W_new                          # the next case starts from a ring slot
    return got, one, W0


def _assert_same_as_one_rank(got, one):
    np.testing.assert_array_equal(got.status, one.status)
    np.testing.assert_array_equal(got.coeffs, one.coeffs)
    _same_bytes(got.W_new, one.W_new, "W_new, several ranks against one")
    np.testing.assert_array_equal(got.cs, one.cs)
    np.testing.assert_array_equal(got.ok, one.ok)


AGG_MASKS = {"all-kept": [1, 1, 1, 1, 1, 1, 1], "mixed": [1, 0, 1, 1, 0, 1, 0], "rank1-all-masked": [0, 1, 1, 0, 0, 0, 0]}


@pytest.mark.parametrize("case", list(AGG_MASKS))
def test_partials_gather_recovery_against_one_rank(two_ctx, shares7, case):
    """Three simulated ranks (4 rows, 3 rows, none: rank 2's commitment slot is the point at infinity) through
    bsc_round_select_partials + the copied gather + bsc_round_after_gather with audit = 1, against the
    Python-integer total and bsc_round_after_select over the same 7 rows on an identically built context."""
    q, pts, ys = shares7
    mask = AGG_MASKS[case]
    got, one, W0 = _three_ranks_then_one(two_ctx, pts, ys, mask)
    total = _coeff_total(q, mask)
    assert got.status.tolist() == [1] * NCH and got.ok.tolist() == [[1] * NCH]
    np.testing.assert_array_equal(got.coeffs, total)
    assert got.clock.tolist() == CLOCKS
    np.testing.assert_allclose(got.W_new, W0 + total.reshape(-1)[:D].astype(np.float64) / QS)
    _assert_same_as_one_rank(got, one)


def test_partials_gather_recovery_corrupt_share(two_ctx, shares7):
    """One share value of a kept row of rank 0 changed: its chunk's recovery fails, on both paths alike."""
    q, pts, ys = shares7
    mask = AGG_MASKS["mixed"]
    bad = ys.clone()
    bad[2, 4, OUTER14[5]] += 1
    got, one, W0 = _three_ranks_then_one(two_ctx, pts, bad, mask)
    want = [int(k != 4) for k in range(NCH)]
    assert got.status.tolist() == want and one.status.tolist() == want
    total = _coeff_total(q, mask)
    total[4] = 0
    np.testing.assert_array_equal(got.coeffs, total)
    np.testing.assert_array_equal(got.W_new[40:50], W0[40:50])
    _assert_same_as_one_rank(got, one)


def test_partials_gather_recovery_swapped_commitment(two_ctx, shares7):
    """One chunk commitment of a kept row of rank 1 replaced by another chunk's: the audit fails for exactly that
    chunk, the recovery does not notice."""
    q, pts, ys = shares7
    mask = AGG_MASKS["mixed"]
    bad = pts.clone()
    bad[5, 6, T] = pts[5, 2, T]
    got, one, _ = _three_ranks_then_one(two_ctx, bad, ys, mask)
    assert got.status.tolist() == [1] * NCH
    assert got.ok.tolist() == [[int(k != 6) for k in range(NCH)]]
    np.testing.assert_array_equal(got.coeffs, _coeff_total(q, mask))
    _assert_same_as_one_rank(got, one)


def test_round_wait_takes_a_slot(two_ctx):
    """bsc_round_wait names what it waits for: 0 the recovery's read-back, 2 / 3 an audit slot.  Anything else --
    the former 1 ("the audit queued last") included -- is refused before an event is touched; nothing is queued or
    launched here."""
    torch.cuda.synchronize()
    for c in (two_ctx.multi, two_ctx.single):
        for which in (1, 4, -1):
            assert hip().bsc_round_wait(c.na.ctx, which) == -1
        assert hip().bsc_round_wait(c.na.ctx, 0) == 0
    assert hip().bsc_round_wait(None, 0) == -1


def test_emulated_collectives(eng, shares7):
    """Rank 0 of 4 alone (every collective one replicate launch): bsc_round_agg_multi leaves rank 0's send pieces in
    every slot of the two-piece receive layout ([world][cs] then [world][ys | clock]), recovers 4 times rank 0's
    total, mirrors the clock 4 times and passes the audit; bsc_round_vg_exchange leaves rank 0's row in every rank's
    row, so the unpacked blocks repeat rank 0's.  None of the replicated pieces is a multiple of 256 words."""
    q, pts, ys = shares7
    world, mask, clock = 4, [1, 0, 1, 1], -1234567890123
    cs_bytes, ys_bytes = 96 * NCH, 8 * NCH * T + 8
    c = _Ctx(eng)
    c2 = _Ctx(eng)
    try:
        na = c.na
        assert na.comm_init(_comm(world)) is True
        send, recv = na.gather_buffers(world)
        maxlocal, num_nodes = 8, 9
        na.bind_multi(maxlocal, num_nodes, vg=None)
        W = torch.from_numpy(np.random.default_rng(4).standard_normal(D)).cuda()
        sp = _handle(pts[:4], ys[:4], mask)
        W_new, pre = na.agg_multi(None, None, sp, -1, c.upload, c.lid, clock, W, 1, -1, True, False)
        assert pre == -1 and W_new.data_ptr() != W.data_ptr()
        got = _results(c, W_new, clocks=True)
        total = _coeff_total(q[:4], mask)
        assert got.status.tolist() == [1] * NCH and got.ok.tolist() == [[1] * NCH]
        np.testing.assert_array_equal(got.coeffs, world * total)
        assert got.clock.tolist() == [clock] * world
        np.testing.assert_allclose(got.W_new, W.cpu().numpy() + world * total.reshape(-1)[:D].astype(np.float64) / QS)
        # rank 0's send row against the references, then every slot of both regions against it
        row = send.cpu().numpy()
        kept = ys.cpu().numpy()[:4][np.asarray(mask, bool)].sum(0, dtype=np.int64)
        _same_bytes(row[cs_bytes:cs_bytes + ys_bytes], np.concatenate([kept.reshape(-1), [clock]]), "send [ys | clock]")
        ref_cs = B.sum_rows(pts[:4].reshape(4, -1, 24), None, c.ccols, row_mask=sp.alive)
        send_cs = torch.from_numpy(row[:cs_bytes].copy()).view(torch.int32).view(NCH, 24).cuda()
        np.testing.assert_array_equal(B.marshal(send_cs).cpu().numpy(), B.marshal(ref_cs).cpu().numpy())
        flat = recv.cpu().numpy().reshape(-1)
        assert (cs_bytes // 4) % 256 and (ys_bytes // 4) % 256
        _same_bytes(flat[:world * cs_bytes], np.tile(row[:cs_bytes], world), "recv [world][cs]")
        _same_bytes(flat[world * cs_bytes:world * (cs_bytes + ys_bytes)],
                    np.tile(row[cs_bytes:cs_bytes + ys_bytes], world), "recv [world][ys | clock]")

        # the verification row through a second context's communicator
        na2 = c2.na
        assert na2.comm_init(_comm(world)) is True
        na2.gather_buffers(world)
        nn, pw = 2, 24
        _, _, chunk, npairs, _ = _own_pairs(world * maxlocal + num_nodes, 0, world)
        assert (chunk, npairs) == (2, 6)
        vg = VerifyGather(_comm(world), maxlocal, pw, nn, chunk, npairs, num_nodes, "cuda")
        vg.native = na2
        na2.bind_multi(maxlocal, num_nodes, vg)
        m = _VgRows(world, maxlocal, nn, pw, chunk, seed=9, ranks=[0])
        assert (vg.commit_off, vg.nz_off, vg.sc_off, vg.row_bytes) == (m.commit_off, m.nz_off, m.sc_off, m.row_bytes)
        assert (m.row_bytes // 4) % 256
        it = 1
        vg.recv[it % 2].copy_(m.start())
        q0 = m.ranks[0]
        commits = torch.from_numpy(q0.commits.view(np.int32)).cuda()
        wrow = [31, 8, 0, 17, 26]
        gram, nz, sc, host, ev = vg.exchange(it, commits, q0.src.tolist(), q0.nz, q0.sc, wrow)
        torch.cuda.synchronize()
        m.model[1:] = m.model[0]             # every rank's row is rank 0's
        m.slots[1:] = m.slots[0]
        m.ranks = m.ranks * world
        _same_bytes(vg.recv[it % 2], m.model, "the replicated verification rows")
        e_gram, e_nz, e_sc, e_commits = m.expect_unpacked(npairs, wrow)
        _same_bytes(gram, e_gram, "tiled Gram")
        _same_bytes(nz, e_nz, "flat noiser ids")
        _same_bytes(sc, e_sc, "flat noiser weights")
        _same_bytes(host.numpy(), e_commits, "pinned commitment rows")
    finally:
        c.close()
        c2.close()
