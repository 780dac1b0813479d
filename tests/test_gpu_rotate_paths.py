"""The restart rotation's four kernels where one workgroup rotates more than one row tile, with a padded V,
and with poison past the columns they may read.

Every case first asks nkv_rotate_plan which kernel and instantiation it is about to run and asserts it, so a
moved threshold fails here instead of quietly testing another kernel.  The multi-trip cases then assert that
the layout has more row tiles than the launch has workgroups (32 resident waves per CU at the most, the
bound the launchers use themselves), so at least one workgroup takes a second tile: the second trip of
k_rotate_chunked reuses its LDS double buffer, k_rotate_wide issues the next tile's first two batches before
this tile's stores, and the streaming kernels restart their batch pipelines.

Reference: numpy float64 V^T Q over the streamed rows, rtol 1e-12 / atol 1e-13 as every rotation test.  For
the k > 256 cases the float64 product was compared once with an np.longdouble-accumulated product of the
same inputs (hashed columns in [-1, 1), V from a QR factor; every 16th row of the layout below, on the CPU):
    (k, n_out)    max |f64 - longdouble|    largest share of the tolerance 1e-13 + 1e-12 |longdouble|
    (440, 20)     2.4e-15                   0.014
    (300, 40)     3.3e-15                   0.013
    (280, 64)     3.4e-15                   0.013
    (620, 20)     2.9e-15                   0.017
    (300, 64)     3.6e-15                   0.013
    (300, 150)    4.1e-15                   0.015
Every share is under a tenth, so the float64 product is the reference for every case.
"""
import ctypes

import numpy as np
import pytest
import torch

from nekstab_next_amd import _lib
from nekstab_next_amd.layout import NekLayout, box3d_layout
from nekstab_next_amd.vector import NekContext, rotate_plan

pytestmark = pytest.mark.gpu

BIG = box3d_layout(120)          # rows = 274432, ld = 278528: four weighted fields + pressure, 3-D
SMALL = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=37, n_scalars=1)   # LAYOUTS["3d_scalar"]: odd sizes, ragged pads


def cu_count():
    n = ctypes.c_int(0)
    _lib.check(_lib.load().nkv_device_info(None, ctypes.byref(n), None, None, 0), "nkv_device_info")
    return n.value


@pytest.fixture(scope="module")
def ctxs(gpu):
    return {id(BIG): NekContext(BIG), id(SMALL): NekContext(SMALL)}


def rotation_inputs(k, n_out, ldv):
    """V: the first n_out columns of a QR factor, column-major at leading dimension ldv; the rows past k
    of every column are NaN (no kernel may read them)."""
    V = np.linalg.qr(np.random.default_rng(1000 * k + n_out).standard_normal((k, k)))[0][:, :n_out]
    Vp = np.full((ldv, n_out), np.nan)
    Vp[:k] = V
    return V, np.asfortranarray(Vp).ravel(order="F")


def rotate(ctx, k, n_out, ldv, seed=500):
    """Columns 0..k-1 hashed (every row differs, so a misplaced tile cannot pass), a distinct time per
    column, column k all NaN.  Returns (before, got, V) on the host."""
    lay = ctx.layout
    Q = ctx.basis(k + 1)
    for i in range(k):
        Q[i].fill_hash(seed + i)
    Q.storage[:k, lay.time_offset] = torch.arange(1, k + 1, dtype=torch.float64, device=ctx.device) * 0.25
    Q.storage[k].fill_(float("nan"))
    before = Q.storage.cpu().numpy()
    V, Vflat = rotation_inputs(k, n_out, ldv)
    Vd = torch.as_tensor(Vflat).to(ctx.device)
    ctx.call("nkv_rotate_cols", Q.ptr, k, Vd.data_ptr(), ldv, n_out, ctx.stream)
    got = Q.storage.cpu().numpy()
    del Q
    return before, got, V


def assert_same_bits(got, want):
    """assert_array_equal, and bit for bit (signed zeros too): the bits are compared first because the
    element-wise report takes seconds on a gigabyte, so it runs only to describe a mismatch."""
    a, b = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64)
    if not np.array_equal(a, b):
        np.testing.assert_array_equal(got, want)
        raise AssertionError("arrays are equal as numbers and differ in bits")


def check_rotation(lay, k, n_out, before, got, V):
    rows = lay.rows   # streamed rows; the time slot and the padding after it are not rotated
    assert not np.isnan(before[:k]).any() and np.isnan(before[k]).all()
    want = V.T @ before[:k, :rows]
    # a load past column k (NaN) would poison an output even where its coefficient is zero
    assert not np.isnan(got[:n_out]).any()
    for i in range(n_out):
        np.testing.assert_allclose(got[i, :rows], want[i], rtol=1e-12, atol=1e-13)
    assert_same_bits(got[:n_out, rows:], before[:n_out, rows:])   # time slot and padding of the kept columns
    assert_same_bits(got[n_out:k], before[n_out:k])               # columns not kept
    assert np.isnan(got[k]).all()                                 # column k: still all NaN


# (path, inst, k, n_out): the loop shape each pair was chosen for
MULTI_TRIP = [
    ("wide", 2, 20, 17),       # two batches, no steady trip
    ("wide", 2, 100, 17),      # one steady trip, k % 16 != 0 (clamped last batch)
    ("wide", 2, 128, 25),      # k % 16 == 0: every batch whole
    ("wide", 3, 130, 48),      # steady trips, then a one-k-row tail batch
    ("wide", 3, 37, 33),       # no steady trip, odd tail
    ("wide", 4, 250, 64),      # four steady trips, partial last batch
    ("stream", 2, 440, 20),    # two-batch pipeline, 16 waves
    ("stream", 3, 300, 40),
    ("stream", 4, 280, 64),    # two-batch pipeline, 8 waves
    ("stream", 5, 83, 70),     # two batches ahead (MB >= 5): no steady trip
    ("stream", 7, 150, 100),   # ... one steady trip and a tail
    ("stream", 8, 128, 128),   # ... k == n_out, whole batches
    ("chunked", 2, 620, 20),   # 32-row k-chunks, 8 waves
    ("chunked", 4, 300, 64),
    ("chunked", 8, 200, 128),
    ("chunked", 12, 300, 150),  # 16-row k-chunks, 4 waves
]


@pytest.mark.parametrize("path,inst,k,n_out", MULTI_TRIP)
def test_rotate_multi_trip(ctxs, path, inst, k, n_out):
    """More row tiles than resident workgroups: the second and later trips of each persistent loop rotate
    the right rows with the right data, touch nothing else, and read nothing past column k."""
    plan = rotate_plan(BIG, k, n_out)
    assert plan[:2] == (path, inst), plan
    _, _, wg_threads, rows_per_tile = plan
    tiles, resident = BIG.rows // rows_per_tile, cu_count() * (2048 // wg_threads)
    print(f"rotate k={k} n_out={n_out}: k_rotate_{path}<{inst}>, {tiles} tiles over at most {resident} workgroups")
    # a device with more CUs needs a larger layout here: fail, never skip
    assert tiles > resident, (tiles, resident)
    before, got, V = rotate(ctxs[id(BIG)], k, n_out, k)
    check_rotation(BIG, k, n_out, before, got, V)


def test_rotate_few_on_the_multi_field_layout(ctxs):
    """k_rotate_few<16> on the same layout.  Its grid is NKV_ROTF_G workgroups of 1024-row tiles whatever the
    device, so this layout's 268 tiles are one band of one trip: the multi-band launch of this kernel is
    tests/test_gpu_kernels.py::test_rotate_cols_row_bands.  Here: the poison and untouched-data assertions."""
    k, n_out = 64, 16
    plan = rotate_plan(BIG, k, n_out)
    assert plan == ("few", 16, 256, 1024), plan
    print(f"rotate k={k} n_out={n_out}: k_rotate_few<16>, {BIG.rows // plan[3]} tiles")
    before, got, V = rotate(ctxs[id(BIG)], k, n_out, k)
    check_rotation(BIG, k, n_out, before, got, V)


@pytest.mark.parametrize("path,inst,k,n_out", [("few", 6, 20, 6), ("few", 12, 35, 12), ("wide", 2, 100, 17),
                                               ("wide", 4, 61, 60), ("stream", 7, 150, 100),
                                               ("stream", 4, 270, 50), ("chunked", 8, 200, 128),
                                               ("chunked", 12, 190, 180)])
def test_rotate_padded_v(ctxs, path, inst, k, n_out):
    """ldv = k + 3 with NaN in rows k..ldv-1 of every V column: the bits of the ldv == k rotation."""
    assert rotate_plan(SMALL, k, n_out, ldv=k + 3)[:2] == rotate_plan(SMALL, k, n_out)[:2] == (path, inst)
    print(f"rotate k={k} n_out={n_out} ldv={k + 3}: k_rotate_{path}<{inst}>")
    ctx = ctxs[id(SMALL)]
    before, dense, V = rotate(ctx, k, n_out, k)
    before_p, padded, Vp = rotate(ctx, k, n_out, k + 3)
    assert_same_bits(before_p, before)
    assert_same_bits(Vp, V)
    check_rotation(SMALL, k, n_out, before_p, padded, Vp)
    assert_same_bits(padded, dense)


def test_plan_and_launcher_refuse_alike(ctxs):
    """nkv_rotate_cols returns nkv_rotate_plan's status for the same bad (k, ldv, n_out)."""
    ctx = ctxs[id(SMALL)]
    lib, Lp = _lib.load(), ctypes.byref(ctx.L)
    Q = ctx.basis(5)
    o = [ctypes.c_int(0) for _ in range(4)]
    for k, ldv, n_out in [(0, 4, 1), (_lib.NKV_MAX_COLS + 1, _lib.NKV_MAX_COLS + 1, 6), (4, 3, 2), (4, 4, 0), (4, 4, 5),
                          (300, 300, _lib.NKV_ROT_MAX_OUT + 1), (600, 600, 600)]:
        want = lib.nkv_rotate_plan(Lp, k, ldv, n_out, *[ctypes.byref(x) for x in o])
        msg = _lib.last_error()
        assert want != _lib.NKV_OK
        assert lib.nkv_rotate_cols(Lp, Q.ptr, k, ctx.h1.data_ptr(), ldv, n_out, ctx.stream) == want
        assert _lib.last_error() == msg
