"""Lane -> (row, chunk, slot) scheduling of the share MSM (k_shares_msm, k_shares_msm_ka), the alive-row compaction
(k_alive_compact) and the signed-digit recode at window boundaries, against the host runtime.

Every device result is compared with ``CommitKey.make_shares`` / ``CommitKey.commit`` of the same coefficient row
(marshalled affine bytes, so a re-ordering of the kernel's additions keeps the tests valid), never only with another
device run.  The host reference of a coefficient row is computed once and shared by every test of this file.

Shapes (poly 10, 21 shares -> 22 lanes per (row, chunk) group, 256-lane blocks, 64-block super-blocks):
  d=101, 70 rows   11 chunks (the last of length 1), 67 blocks: one full super-block plus one of 3 blocks
  d=57,  37 rows   6 chunks, 20 blocks: one partial super-block, 20 % 8 != 0
  d=25,  248 rows  the argument-block kernel's row limit (ROWARG_MAX)
  d=300, 9 rows    30 chunks whose all-zero spans differ between neighbouring rows
  d=21             3 chunks (the last of length 1) of int64 / window-boundary coefficients, b0 in 8, 9, 11, 14
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POLY, T = 10, 21
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

_KEYS: dict = {}     # (d, secret) -> host CommitKey
_ENGS: dict = {}     # (d, secret, b0) -> DeviceCommitEngine
_COEFFS: dict = {}   # case name -> (int64 numpy [P, d], the same on the device)
_REFS: dict = {}     # (id(key), row bytes) -> host reference of one coefficient row


@pytest.fixture(scope="module", autouse=True)
def _release_tables():
    yield
    for eng in _ENGS.values():
        eng.release()
    for cache in (_KEYS, _ENGS, _COEFFS, _REFS):
        cache.clear()


def _setup(rt, d, secret, b0):
    from biscotti_amd.ops import bn256 as B
    if (d, secret) not in _KEYS:
        _KEYS[(d, secret)] = rt.CommitKey.generate(d, secret)
    key = _KEYS[(d, secret)]
    if (d, secret, b0) not in _ENGS:
        _ENGS[(d, secret, b0)] = B.DeviceCommitEngine(key, POLY, T, b0=b0)
    return key, _ENGS[(d, secret, b0)]


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _host_ref(key, row):
    """(witnesses [nch, T, 64], chunk commitments [nch, 64], ys [nch, T], full commitment) of one row, cached."""
    k = (id(key), row.tobytes())
    ref = _REFS.get(k)
    if ref is None:
        commitment, cc, ys, wits = key.make_shares(row, POLY, T)
        nch = len(cc)
        ref = _REFS[k] = (np.frombuffer(b"".join(wits), np.uint8).reshape(nch, T, 64),
                          np.frombuffer(b"".join(cc), np.uint8).reshape(nch, 64),
                          np.array(ys, dtype=np.int64).reshape(nch, T), commitment)
    return ref


def _poison(eng, n, commit_only):
    """The wrappers allocate their outputs uninitialised, and the caching allocator hands a block freed by an
    earlier run straight back -- possibly still holding that run's correct answer.  Fill such blocks with a
    pattern first (and, beyond that, no two runs of this file use the same row list), so a lane that never
    writes its output cannot pass on stale data."""
    S = 1 if commit_only == 1 else T + 1
    a = torch.full((n, eng.nchunks, S, 24), POISON32, dtype=torch.int32, device="cuda")
    b = torch.full((n, eng.nchunks, T), POISON64, dtype=torch.int64, device="cuda")
    del a, b


def _marshalled(eng, pts, ys, commit_only, pos):
    """Device outputs at the list positions `pos` as host arrays: (witness bytes [m, nch, T, 64] or None,
    chunk-commitment bytes [m, nch, 64] or None, ys [m, nch, T] or None)."""
    from biscotti_amd.ops import bn256 as B
    n, nch, m = pts.shape[0], eng.nchunks, len(pos)
    idx = torch.from_numpy(np.asarray(pos, dtype=np.int64)).cuda()
    if commit_only == 1:
        assert tuple(pts.shape) == (n, nch, 1, 24) and ys is None
        return None, B.marshal(pts[idx]).cpu().numpy().reshape(m, nch, 64), None
    assert tuple(pts.shape) == (n, nch, T + 1, 24) and tuple(ys.shape) == (n, nch, T) and ys.dtype == torch.int64
    sel = pts[idx]
    w = B.marshal(sel[:, :, :T].contiguous()).cpu().numpy().reshape(m, nch, T, 64)
    c = None   # commit_only == 2 leaves slot T unwritten
    if commit_only == 0:
        c = B.marshal(sel[:, :, T].contiguous()).cpu().numpy().reshape(m, nch, 64)
    return w, c, ys[idx].cpu().numpy()


def _same(got, exp, what, pos, row_list):
    if np.array_equal(got, exp):
        return
    i = np.argwhere(got != exp)[0]
    raise AssertionError(f"{what} differs from the host at list position {pos[i[0]]} (row {row_list[pos[i[0]]]}), "
                         f"chunk {i[1]}, index {tuple(int(v) for v in i[2:])};{int((got != exp).any(-1).sum())} entries differ")


def _check_against_host(key, eng, coeffs_np, row_list, pts, ys, commit_only, live=None):
    """Every live list position's witnesses, chunk commitments and share values (what `commit_only` computes) equal
    the host's make_shares of that coefficient row.  Returns the number of positions checked."""
    row_list = np.asarray(row_list)
    pos = np.arange(len(row_list)) if live is None else np.flatnonzero(np.asarray(live))
    if len(pos) == 0:
        return 0
    refs = [_host_ref(key, coeffs_np[row_list[p]]) for p in pos]
    w, c, y = _marshalled(eng, pts, ys, commit_only, pos)
    if w is not None:
        _same(w, np.stack([r[0] for r in refs]), "witness", pos, row_list)
        _same(y[..., None], np.stack([r[2] for r in refs])[..., None], "share value", pos, row_list)
    if c is not None:
        _same(c, np.stack([r[1] for r in refs]), "chunk commitment", pos, row_list)
    return len(pos)


def _random_case(rt, d, n, b0=8, secret=3):
    """n distinct random rows with |c| < 2^13 (the workload's quantised update range)."""
    key, eng = _setup(rt, d, secret, b0)
    name = ("random", d, n)
    if name not in _COEFFS:
        c = np.random.default_rng(1000 * d + n).integers(-(2**13) + 1, 2**13, size=(n, d), dtype=np.int64)
        assert len({r.tobytes() for r in c}) == n
        _COEFFS[name] = (c, torch.from_numpy(c).cuda())
    return (key, eng) + _COEFFS[name]


def _permuted(n, *what):
    return np.random.default_rng(_seed(*what)).permutation(n).astype(np.int32)


# ------------------------------------------------------------------ a. large grids with group_rows
_SCHEDULES = [(0, 0), (1, 0), (8, 0), (21, 0), ("n", 0), ("n+5", 0), (0, 1), (0, 2), (8, 1), (8, 2)]


@pytest.mark.parametrize("G,commit_only", _SCHEDULES, ids=[f"G{g}-co{c}" for g, c in _SCHEDULES])
@pytest.mark.parametrize("d,n", [(101, 70), (57, 37)])
def test_group_rows_large_grid(rt, d, n, G, commit_only):
    key, eng, coeffs, ct = _random_case(rt, d, n)
    nblocks = -(-n * eng.nchunks * (T + 1) // 256)
    assert (d, nblocks) in ((101, 67), (57, 20)) and nblocks % 8 != 0   # the grids this test is about
    rows = _permuted(n, "a", d, n, G, commit_only)
    group_rows = {"n": n, "n+5": n + 5}.get(G, G)
    _poison(eng, n, commit_only)
    pts, ys = eng.shares(ct, torch.from_numpy(rows).cuda(), commit_only=commit_only, group_rows=group_rows)
    assert _check_against_host(key, eng, coeffs, rows, pts, ys, commit_only) == n


# ------------------------------------------------------------------ b. compaction and pre-cleared flags
def _flag_pattern(name, n):
    m = np.zeros(n, dtype=np.int32)
    if name == "all":
        m[:] = 1
    elif name == "alternating":
        m[::2] = 1
    elif name == "last":
        m[-1] = 1
    elif name == "first":
        m[0] = 1
    elif name == "random-half":
        m[np.random.default_rng(11).permutation(n)[:n // 2]] = 1
    else:
        assert name == "none"
    return m


_FLAG_MODES = [(True, 0), (True, 8), (False, 8)]   # (compact, group_rows); not compact: per-thread skip
_FLAG_IDS = ["compact-G0", "compact-G8", "skip-G8"]


@pytest.mark.parametrize("compact,G", _FLAG_MODES, ids=_FLAG_IDS)
@pytest.mark.parametrize("pattern", ["all", "alternating", "last", "first", "random-half"])
def test_flagged_rows(rt, pattern, compact, G):
    d, n = 57, 37
    key, eng, coeffs, ct = _random_case(rt, d, n)
    mask = _flag_pattern(pattern, n)
    rows = _permuted(n, "b", pattern, compact, G)
    _poison(eng, n, 0)
    pts, ys = eng.shares(ct, torch.from_numpy(rows).cuda(), alive=torch.from_numpy(mask).cuda(), compact=compact,
                         group_rows=G)
    checked = _check_against_host(key, eng, coeffs, rows, pts, ys, 0, live=mask)
    assert checked == mask.sum() and checked > 0


@pytest.mark.parametrize("compact,G", _FLAG_MODES, ids=_FLAG_IDS)
def test_no_flagged_row(rt, compact, G):
    """Every flag cleared: the outputs are undefined; the launch must succeed and the stream must drain."""
    d, n = 57, 37
    key, eng, coeffs, ct = _random_case(rt, d, n)
    rows = _permuted(n, "b", "none", compact, G)
    eng.shares(ct, torch.from_numpy(rows).cuda(), alive=torch.from_numpy(_flag_pattern("none", n)).cuda(),
               compact=compact, group_rows=G)    # raises unless bsc_shares_msm returned 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ c. k_alive_compact alone
@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 1500, 4096])
def test_alive_compact(n, kind):
    from biscotti_amd.native import hip
    from biscotti_amd.ops import bn256 as B
    if kind == "random":   # any non-zero flag counts as alive
        flags = np.random.default_rng(n).choice(np.array([0, 0, 1, 3, -1], dtype=np.int32), size=n)
        flags[-1] = 2   # the last thread's last row always counts (the all-zero case has it cleared)
    else:
        flags = np.full(n, 1 if kind == "ones" else 0, dtype=np.int32)
    alive = torch.from_numpy(flags).cuda()
    out = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    assert hip().bsc_alive_compact(alive.data_ptr(), n, out.data_ptr(), B._stream()) == 0
    got = out.cpu().numpy()
    want = np.flatnonzero(flags)
    assert got[0] == len(want) == (flags != 0).sum()
    np.testing.assert_array_equal(got[1:1 + len(want)], want)
    assert (got[1 + len(want):] == -7).all()   # nothing written behind the list


def test_alive_compact_rejects_more_than_one_block_can_scan():
    from biscotti_amd.native import hip
    from biscotti_amd.ops import bn256 as B
    alive = torch.ones(4097, dtype=torch.int32, device="cuda")
    out = torch.full((4098,), -7, dtype=torch.int32, device="cuda")
    assert hip().bsc_alive_compact(alive.data_ptr(), 4097, out.data_ptr(), B._stream()) == -1
    assert (out.cpu().numpy() == -7).all()


# ------------------------------------------------------------------ d. the argument-block kernel
def _ka_case(rt):
    d = 25
    key, eng = _setup(rt, d, 3, 8)
    if "ka" not in _COEFFS:
        c = np.random.default_rng(25).integers(-(2**13) + 1, 2**13, size=(12, d), dtype=np.int64)
        _COEFFS["ka"] = (c, torch.from_numpy(c).cuda())
    return (key, eng) + _COEFFS["ka"]


def _ka_list(n, *what):
    """n entries over the 12 coefficient rows, adjacent entries always different."""
    rng = np.random.default_rng(_seed("d", *what))
    lst = np.empty(n, dtype=np.int32)
    lst[0] = rng.integers(12)
    for i in range(1, n):
        lst[i] = (lst[i - 1] + rng.integers(1, 12)) % 12
    assert (lst[1:] != lst[:-1]).all() and len(set(lst.tolist())) == 12
    return lst


@pytest.mark.parametrize("with_alive", [False, True], ids=["all-rows", "alive"])
@pytest.mark.parametrize("commit_only", [0, 2])
@pytest.mark.parametrize("G", [0, 16])
def test_shares_ka_at_row_limit(rt, G, commit_only, with_alive):
    from biscotti_amd.ops import bn256 as B
    n = B.NativeSecAgg.ROWARG_MAX
    assert n == 248
    key, eng, coeffs, ct = _ka_case(rt)
    lst = _ka_list(n, G, commit_only, with_alive)
    mask = alive = None
    if with_alive:
        mask = (np.random.default_rng(_seed("d-alive", G, commit_only)).random(n) < 0.5).astype(np.int32)
        mask[-1] = 1   # the last argument-block entry stays live
        alive = torch.from_numpy(mask).cuda()
    _poison(eng, n, commit_only)
    pts, ys = eng.shares_ka(ct, lst, commit_only=commit_only, alive=alive, group_rows=G)
    checked = _check_against_host(key, eng, coeffs, lst, pts, ys, commit_only, live=mask)
    assert checked == (n if mask is None else mask.sum()) and checked > 0
    # the device-list kernel on the same list
    pts2, ys2 = eng.shares(ct, torch.from_numpy(lst).cuda(), commit_only=commit_only, alive=alive, group_rows=G)
    pos = np.arange(n) if mask is None else np.flatnonzero(mask)
    for a, b in zip(_marshalled(eng, pts, ys, commit_only, pos), _marshalled(eng, pts2, ys2, commit_only, pos)):
        assert (a is None and b is None) or np.array_equal(a, b)


def test_shares_ka_rejects_rows_beyond_argument_block(rt):
    from biscotti_amd.native import hip
    from biscotti_amd.ops import bn256 as B
    key, eng, coeffs, ct = _ka_case(rt)
    n = 249
    lst = np.ascontiguousarray(np.arange(n, dtype=np.int32) % 12)
    pts = torch.full((n, eng.nchunks, T + 1, 24), POISON32, dtype=torch.int32, device="cuda")
    ys = torch.full((n, eng.nchunks, T), POISON64, dtype=torch.int64, device="cuda")
    err = hip().bsc_shares_msm_ka(ct.data_ptr(), eng.d, lst.ctypes.data, n, eng.tbl_pk.data_ptr(),
                                  eng.tbl_wb.data_ptr(), POLY, T, eng.b0, eng.nw, 0, None, 0, pts.data_ptr(),
                                  ys.data_ptr(), B._stream())
    assert err == -1
    torch.cuda.synchronize()
    assert bool((pts == POISON32).all()) and bool((ys == POISON64).all())   # nothing was launched
    with pytest.raises(RuntimeError):
        eng.shares_ka(ct, lst)


# ------------------------------------------------------------------ e. digit and int64 edges through recode()
# These cases pin the digit range to what the tables hold, |digit| <= 2^(bits-1).  They cannot tell a carry at
# digit == 2^(bits-1) from one above it: -2^(bits-1) selects an existing entry too, and |c| <= 2^63 keeps the top
# window's digit below 66, so both recodings give the same point.  A carry threshold one higher fails them.
EDGE_B0 = [8, 9, 11, 14]   # b0 = 9: the windows cover exactly 65 bits, no slack for a carry into the top window
EDGE_D, EDGE_SECRET = 21, 2


def _edge_case(rt, b0):
    key, eng = _setup(rt, EDGE_D, EDGE_SECRET, b0)
    name = ("edge", b0)
    if name not in _COEFFS:
        h = 1 << (b0 - 1)   # the largest first-window digit
        vals = [h, -h, h + 1, -(h + 1), (1 << b0) - 1, 1 << b0, 128 << b0, 129 << b0, (1 << 63) - h,
                0x7f7f7f7f7f7f7f7f, -0x0080808080808080, I64_MAX, I64_MIN, I64_MIN + 1, 1, -1, 0]
        vals += [129 << b0, h + 1, I64_MAX, I64_MIN]   # pad to d = 21; the length-1 last chunk holds INT64_MIN
        assert len(vals) == EDGE_D
        neg = [v if v == I64_MIN else -v for v in vals]
        c = np.array([vals, neg], dtype=np.int64)
        _COEFFS[name] = (c, torch.from_numpy(c).cuda())
    return (key, eng) + _COEFFS[name]


@pytest.mark.parametrize("commit_only", [0, 1, 2])
@pytest.mark.parametrize("b0", EDGE_B0)
def test_digit_edges_shares(rt, b0, commit_only):
    key, eng, coeffs, ct = _edge_case(rt, b0)
    rows = np.array([1, 0], dtype=np.int32) if commit_only == 1 else np.array([0, 1], dtype=np.int32)
    _poison(eng, 2, commit_only)
    pts, ys = eng.shares(ct, torch.from_numpy(rows).cuda(), commit_only=commit_only)
    assert _check_against_host(key, eng, coeffs, rows, pts, ys, commit_only) == 2


@pytest.mark.parametrize("b0", EDGE_B0)
def test_digit_edges_full_commitments(rt, b0):
    """k_commit_rows and the sum of k_shares_msm's chunk commitments against the host's commit and against
    (sum_i c_i s^i) G computed with Python integers (PK[i] = s^i G)."""
    from biscotti_amd.ops import bn256 as B
    key, eng, coeffs, ct = _edge_case(rt, b0)
    rows = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    by_rows = B.marshal(eng.commit_rows(ct, rows)).cpu().numpy()
    pts, _ = eng.shares(ct, rows)
    by_chunks = B.marshal(eng.commitments(pts)).cpu().numpy()
    order, g = rt.bn256_order(), rt.g1_generator()
    for i, r in enumerate([1, 0]):
        scalar = sum(int(c) * EDGE_SECRET**j for j, c in enumerate(coeffs[r])) % order
        want = rt.g1_mul(g, scalar)
        assert key.commit(coeffs[r], 0) == want == _host_ref(key, coeffs[r])[3]
        assert bytes(by_rows[i]) == want, ("commit_rows", r)
        assert bytes(by_chunks[i]) == want, ("sum of chunk commitments", r)


@pytest.mark.parametrize("b0", EDGE_B0)
def test_digit_edges_chunk_check(rt, b0):
    """k_chunk_check with the edge coefficients as the recovered chunks: every chunk matches the commit-only pass's
    commitments (themselves checked against the host), and changing one coefficient by one clears that chunk's
    flag only."""
    key, eng, coeffs, ct = _edge_case(rt, b0)
    nch = eng.nchunks
    for r in (0, 1):
        pts, _ = eng.shares(ct, torch.tensor([r], dtype=torch.int32, device="cuda"), commit_only=1)
        assert _check_against_host(key, eng, coeffs, [r], pts, None, 1) == 1
        csum = pts.view(1, nch, 24)
        rec = np.zeros((nch, POLY), dtype=np.int64)
        rec.reshape(-1)[:EDGE_D] = coeffs[r]
        assert eng.check_chunks(torch.from_numpy(rec).cuda(), csum).cpu().numpy().tolist() == [[1] * nch]
        for k in range(nch):
            L = min(POLY, EDGE_D - POLY * k)
            for j in sorted({0, L - 1}):
                bad = rec.copy()
                bad[k, j] += -1 if bad[k, j] == I64_MAX else 1
                want = [[int(c != k) for c in range(nch)]]
                assert eng.check_chunks(torch.from_numpy(bad).cuda(), csum).cpu().numpy().tolist() == want, (r, k, j)


# ------------------------------------------------------------------ f. class-row-structured sparsity
SPARSE_D, SPARSE_N, ZERO_ROW, C0_ROW = 300, 9, 7, 8


def _sparse_case(rt):
    key, eng = _setup(rt, SPARSE_D, 3, 8)
    if "sparse" not in _COEFFS:
        rng = np.random.default_rng(300)
        nch = SPARSE_D // POLY
        shape = (SPARSE_N, nch, POLY)
        c = rng.integers(1, 2**13, size=shape, dtype=np.int64) * rng.choice([-1, 1], size=shape)
        for r in range(SPARSE_N):
            for k in range(nch):
                if (r + k // 5) % 3 == 0:   # rows r, r+1, r+2 share a wave: exactly one of them idles at chunk k
                    c[r, k] = 0
        c[ZERO_ROW] = 0
        c[C0_ROW, :, 1:] = 0
        c[C0_ROW, :, 0] = rng.integers(1, 2**13, size=nch) * rng.choice([-1, 1], size=nch)
        c = np.ascontiguousarray(c.reshape(SPARSE_N, SPARSE_D))
        _COEFFS["sparse"] = (c, torch.from_numpy(c).cuda())
    return (key, eng) + _COEFFS["sparse"]


@pytest.mark.parametrize("G,compact", [(0, False), (3, False), (0, True), (3, True)],
                         ids=["G0", "G3", "compact-G0", "compact-G3"])
def test_class_row_structured_sparsity(rt, G, compact):
    key, eng, coeffs, ct = _sparse_case(rt)
    n, nch = SPARSE_N, eng.nchunks
    assert nch == 30
    # a rotation per run keeps neighbouring rows neighbours in the list
    rows = np.roll(np.arange(n, dtype=np.int32), -(1 + 2 * G + int(compact)))
    mask = alive = None
    if compact:
        mask = (~np.isin(rows, [1, 4])).astype(np.int32)
        alive = torch.from_numpy(mask).cuda()
    _poison(eng, n, 0)
    pts, ys = eng.shares(ct, torch.from_numpy(rows).cuda(), alive=alive, compact=compact, group_rows=G)
    assert _check_against_host(key, eng, coeffs, rows, pts, ys, 0, live=mask) == (n - 2 if compact else n)
    # the two degenerate rows, spelled out
    pz, pc = int(np.flatnonzero(rows == ZERO_ROW)[0]), int(np.flatnonzero(rows == C0_ROW)[0])
    w, c, y = _marshalled(eng, pts, ys, 0, [pz, pc])
    assert not w[0].any() and not c[0].any() and not y[0].any()   # infinity marshals to zeros
    assert not w[1].any() and c[1].any(-1).all()                   # no witness, a commitment in every chunk
    np.testing.assert_array_equal(y[1], np.broadcast_to(coeffs[C0_ROW].reshape(nch, POLY)[:, :1], (nch, T)))
