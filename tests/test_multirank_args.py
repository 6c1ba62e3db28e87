"""Argument checks of the multi-rank round's launchers (kernels/gather.hip, the strided recovery and the tail sums
of kernels/ml.hip, the packed row length of kernels/round.hip).

Only paths that return before any launch: the library loads without a GPU (the HIP runtime initialises lazily, as
test_abi_symbols.py relies on), so these run in the CPU suite.  The kernels themselves are compared with their
references in test_gpu_multirank_pieces.py.
"""
import ctypes

import numpy as np
import pytest

from biscotti_amd.native import hip
from biscotti_amd.ops.gather import VerifyGather, limits

NCH, T, POLY = 9, 21, 10   # d = 85: the shape the GPU file runs


@pytest.mark.parametrize("nch", [1, 9, 785])
@pytest.mark.parametrize("t", [1, 21])
def test_round_row_bytes_is_the_padded_row(nch, t):
    """[cs: nch x 24 u32 | ys: nch x T int64 | clock: int64], padded to whole 96-byte points and no further."""
    raw = 96 * nch + 8 * nch * t + 8
    rb = hip().bsc_round_row_bytes(nch, t)
    assert rb % 96 == 0
    assert raw <= rb < raw + 96


def test_vg_limits_and_fits_agree():
    assert limits() == (128, 256, 1024)
    slots, nz, workers = limits()
    assert VerifyGather.fits(slots, 1, 1) and not VerifyGather.fits(slots + 1, 1, 1)
    assert VerifyGather.fits(1, nz, 1) and not VerifyGather.fits(1, nz + 1, 1)
    assert VerifyGather.fits(slots, nz // slots, 1) and not VerifyGather.fits(slots, nz // slots + 1, 1)
    assert VerifyGather.fits(1, 1, workers) and not VerifyGather.fits(1, 1, workers + 1)


@pytest.mark.parametrize("maxlocal,pw,nnz", [(129, 24, 1), (1, 24, 257), (0, 24, 0), (1, 0, 1)],
                         ids=["maxlocal=129", "nnz=257", "maxlocal=0", "pw=0"])
def test_vg_pack_rejects(maxlocal, pw, nnz):
    src = np.zeros(256, np.int32)
    nz = np.zeros(512, np.int32)
    sc = np.zeros(512, np.float32)
    assert hip().bsc_vg_pack(None, 0, 0, 0, None, maxlocal, pw, src.ctypes.data, nz.ctypes.data, sc.ctypes.data, nnz,
                             None) == -1


def _unpack(world=3, maxlocal=5, nw=1, npairs=10, chunk=4, wrow=None):
    w = np.zeros(2048, np.int32)
    if wrow is not None:
        w[:len(wrow)] = wrow
    return hip().bsc_vg_unpack(None, 4096, chunk, npairs, 0, 0, 0, maxlocal, 24, 2, world, w.ctypes.data, nw, None,
                               None, None, None, None)


def test_vg_unpack_rejects():
    assert _unpack(nw=1025) == -1
    assert _unpack(world=0) == -1
    assert _unpack(npairs=1, chunk=0) == -1
    # a worker row outside the gathered [world * maxlocal] rows
    assert _unpack(wrow=[15]) == -2
    assert _unpack(wrow=[-1]) == -2
    assert _unpack(nw=3, wrow=[14, 0, 15]) == -2


def _recover(nrows=4, rstride=NCH * T + 3, npts=21, poly=POLY, h_clock=False):
    clock = (ctypes.c_longlong * 512)()   # never written: every case returns before the launch
    return hip().bsc_recover_w_clock(None, nrows, rstride, NCH, T, None, None, None, npts, None, None, poly, 0, 1, 0,
                                     85, None, 1e4, None, None, None, None, None, None,
                                     ctypes.addressof(clock) if h_clock else None, None)


def test_recover_w_clock_rejects():
    assert _recover(rstride=NCH * T - 1) == -1               # rows overlap
    assert _recover(rstride=NCH * T, h_clock=True) == -1     # no room for the clock word behind the sums
    assert _recover(nrows=257, h_clock=True) == -1           # block 0 mirrors one clock per thread
    assert _recover(poly=10, npts=9) == -1
    assert _recover(npts=33) == -1


def test_sum_rows_i64_tail_rejects_rows_without_data():
    out = (ctypes.c_longlong * 8)()
    assert hip().bsc_sum_rows_i64_tail(None, 1, 4, None, ctypes.addressof(out), 7, None) == -1
    assert list(out) == [0] * 8
