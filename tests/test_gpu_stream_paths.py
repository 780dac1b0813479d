"""The streaming Gram–Schmidt kernels, BLAS-1 and the finish kernel on the loop shapes the 16-18-tile layouts of
tests/test_gpu_kernels.py never reach: second and later trips of a workgroup, the large (8-pair) tiles, row-band
launches that add into the same partial slots, and the per-unit loop of the DCGS2 update with more work units
than workgroups.  Each result is compared with float64 numpy on the downloaded arrays.

Every case first asks nkv_stream_plan for the shape it is about to run and asserts it, so a moved threshold
fails here instead of quietly testing another loop.  Cases that claim a second trip assert tiles > grid (or
units > grid); cases that claim bands assert launches >= 2.  A claim that no longer holds fails, never skips.

Layouts (ragged padding in every segment; the smallest that reach the paths):
    layout               rows        MB/vector  what it reaches
    box3d_layout(70)     163,840     1.3        1280 128-row tiles: second and third trips of k_update_dot on both
                                                grid caps (1024 and 512)
    box3d_layout(1203)   2,736,128   22         1336 2048-row tiles, 302 per field: the grid-stride loops of
                                                k_axpy_dot, k_block_update<4>, k_block_dot<4> (128 x 4 grid),
                                                k_block_dot2<4> and the per-tile norm loop of k_dcgs2_update<4, true>
    box3d_layout(7501)   16,990,208  136        4148 4096-row tiles, 938 per field, 396 pressure: k_block_dot<8>,
                                                k_block_update<8> on the 4096 grid (52 second-trip tiles) and in bands
                                                2048 + 2048 + 52, k_dcgs2_update<8, false> in bands 1536 + 1536 + 1076,
                                                k_dcgs2_update<8, true> over 1334 work units on 768 workgroups,
                                                k_blas1 / k_finish over 8296 chunks on 4096 workgroups

Shared conditions: columns are hashed (every row differs, so a misplaced tile cannot pass), each column has its
own time, the column after the last one read is all NaN (no output may hold a NaN; that column is still all NaN
afterwards), padding rows of every written vector stay zero, the time slot and the padding after it keep their
bits unless the flag asks for the update, and columns only read keep their bits.

Tolerances are the suite's: vectors rtol 1e-12 / atol 1e-13, dots rtol 1e-12 with atol 1e-12 max|ref|, norm rtol
1e-12, axpby 3 ulp of 2.  The float64 numpy reference was compared once, on the CPU, with an
np.longdouble-accumulated one on the same inputs (host twins of the hashed columns; dots and norms in full,
vector updates on every 16th row); the largest share of the tolerance it consumes:
    case (layout, largest over its column counts)          max |f64 - longdouble|   largest share of the tolerance
    22 MB   block dot, j = 1, 5, 9                          2.4e-14                  0.003
    22 MB   block update j = 2, 5: vector / norm            4.2e-16 / 5.0e-12        0.001 / 0.000
    22 MB   overwrite j = 2, 5: vector                      2.3e-16                  0.001
    22 MB   two-vector dot j = 2, 7, x separate / last      4.9e-14 / 3.2e-11        0.001 / 0.001
    22 MB   axpy_dot: vector / dot with qb / without        1.4e-16 / 2.5e-16 / 6.9e-12   0.000
    22 MB   DCGS2 update m = 9: qbar / f / norm             1.6e-16 / 7.6e-16 / 1.1e-12   0.000 / 0.003 / 0.000
    136 MB  block dot, j = 1, 5                             3.2e-13                  0.013
    136 MB  block update j = 2, 5: vector / norm            4.5e-16 / 7.7e-11        0.001 / 0.001
    136 MB  overwrite j = 2, 5: vector                      2.6e-16                  0.001
    136 MB  DCGS2 update m = 0, 1, 9: qbar / f / norm       1.6e-16 / 8.6e-16 / 4.3e-11   0.000 / 0.003 / 0.001
    1.3 MB  fused pass j = 13, 100, 256: vector / dots      2.3e-13 / 3.8e-11        0.019 / 0.000
Every share is under a tenth, so float64 numpy is the reference for every case.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from nekstab_next_amd import _lib
from nekstab_next_amd import synthetic as syn
from nekstab_next_amd._lib import NKV_NORM2, NKV_OVERWRITE, NKV_TIME, NKV_TIME_DOT, NKV_X_IS_LAST
from nekstab_next_amd.layout import box3d_layout
from nekstab_next_amd.vector import NekContext, stream_plan

pytestmark = pytest.mark.gpu

FUSE = box3d_layout(70)        # rows = 163,840
MID = box3d_layout(1203)       # rows = 2,736,128
BIG = box3d_layout(7501)       # rows = 16,990,208
SEED_Q, SEED_F, SEED_G = 1000, 77, 78
F_TIME, G_TIME = 0.5, -0.7
FUSE_J = (2, 12, 13, 16, 32, 33, 64, 100, 128, 129, 200, 256)


# ---- inputs as plain numpy (the CPU study of the reference's own error uses the same) -----------------------
def weights(lay):
    return syn.sponge(syn.mass_weights(lay))   # zero weights inside a sponge


def col_time(i):
    return 0.25 * (i + 1)


def coeffs(j):
    """Projection coefficients: O(1), no two equal, none zero."""
    return np.linspace(-0.3, 0.7, j) + 0.013


def dcgs2_coef(m):
    """nkv_dcgs2_update's coefficient block [x (m) | c (m+1) | rinv, y, ., s | a (m)]: (coef, a, x, rinv, yc, sc)."""
    rng = np.random.default_rng(m)
    a, x = rng.standard_normal(m) * 1e-2, rng.standard_normal(m) * 0.3
    rinv, yc, sc = 1.0 / 1.0003, 0.27, 1.0 / 1.7
    coef = np.zeros(3 * m + 8)
    coef[:m] = x
    coef[2 * m + 1], coef[2 * m + 2], coef[2 * m + 4] = rinv, yc, sc
    coef[2 * m + 5: 3 * m + 5] = a
    return coef, a, x, rinv, yc, sc


def wfull(lay, w):
    wf = np.zeros(lay.ld)
    for f_ in range(lay.n_wf):
        wf[f_ * lay.sv: f_ * lay.sv + lay.n_v] = w
    return wf


# ---- one context, basis and pair of vectors per layout, built once ----------------------------------------------
class Env:
    """Columns 0..K-1 hashed with distinct times, a pristine device copy of them (Q0) and a host copy (Qh); vectors
    f and g with pristine copies.  A case poisons the column after the last one it reads and restores it."""

    def __init__(self, lay, K):
        self.lay, self.K = lay, K
        self.w = weights(lay)
        self.ctx = NekContext(lay, weights=self.w, max_cols=max(K, 16))
        self.wf = wfull(lay, self.w)
        self.Q = self.ctx.basis(K + 1)
        for i in range(K + 1):
            self.Q[i].fill_hash(SEED_Q + i)
        t = torch.tensor([col_time(i) for i in range(K + 1)], dtype=torch.float64, device=self.ctx.device)
        self.Q.storage[:, lay.time_offset] = t
        self.Q0 = self.Q.storage.clone()
        self.Qh = self.Q0[:K].cpu().numpy()
        self.f, self.g, self.out = self.ctx.vector(), self.ctx.vector(), self.ctx.vector()
        self.f.fill_hash(SEED_F)
        self.g.fill_hash(SEED_G)
        self.f.time, self.g.time = F_TIME, G_TIME
        self.f0, self.g0 = self.f.storage.clone(), self.g.storage.clone()
        self.fh, self.gh = self.f0.cpu().numpy(), self.g0.cpu().numpy()

    def reset(self):
        self.f.storage.copy_(self.f0)
        self.g.storage.copy_(self.g0)
        self.out.storage.zero_()

    @contextlib.contextmanager
    def poisoned(self, j, written=()):
        """Column j all NaN during the call; afterwards columns < j (but the `written` ones) keep their bits and
        column j is still all NaN.  The basis is pristine again on exit."""
        Q, Q0 = self.Q.storage, self.Q0
        self.reset()
        Q[j].fill_(float("nan"))
        try:
            yield
            for c in range(j):
                if c not in written:
                    assert torch.equal(Q[c].view(torch.int64), Q0[c].view(torch.int64)), f"column {c} changed"
            assert bool(torch.isnan(Q[j]).all()), f"column {j} is no longer all NaN"
        finally:
            Q[j].copy_(Q0[j])
            for c in written:
                Q[c].copy_(Q0[c])

    def upload(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.ctx.device)


_envs = {}


def env_of(lay, K):
    if id(lay) not in _envs:
        _envs[id(lay)] = Env(lay, K)
    assert _envs[id(lay)].K >= K
    return _envs[id(lay)]


@pytest.fixture(scope="module", autouse=True)
def _release(gpu):
    torch.cuda.reset_peak_memory_stats()
    yield
    _envs.clear()
    print(f"\npeak device memory of this module: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


@pytest.fixture
def fuse(gpu):
    return env_of(FUSE, max(FUSE_J))


@pytest.fixture
def mid(gpu):
    return env_of(MID, 10)


@pytest.fixture
def big(gpu):
    return env_of(BIG, 10)     # 11 columns with the poisoned one


# ---- assertions ---------------------------------------------------------------------------------------------------
def assert_same_bits(got, want):
    """Bit for bit (signed zeros and NaNs too); the element-wise report runs only to describe a mismatch."""
    a, b = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64)
    if not np.array_equal(a, b):
        np.testing.assert_array_equal(got, want)
        raise AssertionError("arrays are equal as numbers and differ in bits")


def check_vector(lay, got, want_rows, before, time_want=None, exact=False, atol=1e-13, rtol=1e-12):
    """A written vector: the streamed rows against the reference, zero padding rows, and the time slot (against
    time_want where the flag asks for its update, its old bits otherwise) with the padding after it untouched."""
    rows = lay.rows
    assert not np.isnan(got).any()
    if exact:
        assert_same_bits(got[:rows], want_rows)
    else:
        np.testing.assert_allclose(got[:rows], want_rows, rtol=rtol, atol=atol)
    for name, s, n in lay.field_slices():
        assert not got[s + n: s + (lay.sp if name == "pr" else lay.sv)].any(), f"padding rows of {name}"
    if time_want is None:
        assert_same_bits(got[rows:], before[rows:])
    else:
        if exact:
            assert got[rows] == time_want
        else:
            np.testing.assert_allclose(got[rows], time_want, rtol=rtol, atol=atol)
        assert_same_bits(got[rows + 1:], before[rows + 1:])


def check_dots(got, ref):
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


# ---- references ---------------------------------------------------------------------------------------------------
def ref_update(e, j, h, f):
    """f - Q[:, :j] h over every stored row and the time slot."""
    return f - h @ e.Qh[:j]


def ref_dot(e, j, f, time):
    t = e.lay.time_offset
    return e.Qh[:j] @ (e.wf * f) + (e.Qh[:j, t] * f[t] if time else 0.0)


def ref_norm(e, f):
    return float(np.sum(e.wf * f * f))


# ---- fused update + dot: later trips of k_update_dot<NW, CPW> ------------------------------------------------------
@pytest.mark.parametrize("j", FUSE_J)
def test_update_dot_later_trips(fuse, j):
    """4, 8 and 16 waves, both grid caps, CPW slots past j (j = 13, 100, 129, 200): the workgroups that take a
    second (1024 grid) or a second and a third (512 grid) 128-row tile reuse the double-buffered LDS partials with
    one barrier per tile."""
    e, lay = fuse, FUSE
    p = stream_plan(lay, "update_dot", j)
    nw = 4 if j <= 12 else 8 if j <= 128 else 16
    grid = 512 if 16 <= j <= 32 else 1024
    assert (p.kernel, p.nw, p.cpw, p.grid_x, p.tiles, p.launches) == ("update_dot", nw, -(-j // nw), grid, 1280, 1), dict(p)
    assert p.tiles > p.grid_x and (grid == 1024 or p.tiles > 2 * p.grid_x)
    print(f"update_dot j={j}: k_update_dot<{p.nw},{p.cpw}>, {p.tiles} tiles over {p.grid_x} workgroups")
    ctx = e.ctx
    h = coeffs(j)
    hd, hout = e.upload(h), torch.full((j + 1,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(j):
        ctx.call("nkv_block_update_dot", ctx.w.data_ptr(), e.Q.ptr, j, hd.data_ptr(), e.f.ptr, hout.data_ptr(),
                 ctx.ws.data_ptr(), NKV_TIME | NKV_TIME_DOT, ctx.stream)
        got, ho = e.f.to_packed(), hout.cpu().numpy()
    fref = ref_update(e, j, h, e.fh)
    check_vector(lay, got, fref[:lay.rows], e.fh, time_want=fref[lay.time_offset])
    check_dots(ho[:j], ref_dot(e, j, fref, True))
    assert ho[j] == -3.0


# ---- block dot ---------------------------------------------------------------------------------------------------
def run_block_dot(e, j, pairs, grid):
    lay, ctx = e.lay, e.ctx
    p = stream_plan(lay, "block_dot", j)
    assert (p.kernel, p.pairs, p.grid_x, p.grid_y, p.launches) == ("block_dot", pairs, grid, lay.n_wf, 1), dict(p)
    assert p.tiles > p.grid_x, dict(p)
    print(f"block_dot j={j}: k_block_dot<{p.pairs}>, {p.tiles} tiles per field over {p.grid_x} x {p.grid_y} workgroups")
    hout = torch.full((j + 1,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(j):
        ctx.call("nkv_block_dot", ctx.w.data_ptr(), e.Q.ptr, j, e.f.ptr, hout.data_ptr(), ctx.ws.data_ptr(), NKV_TIME,
                 ctx.stream)
        ho = hout.cpu().numpy()
        assert torch.equal(e.f.storage.view(torch.int64), e.f0.view(torch.int64))
    check_dots(ho[:j], ref_dot(e, j, e.fh, True))
    assert ho[j] == -3.0


@pytest.mark.parametrize("j", [1, 5, 9])
def test_block_dot_grid_stride_small_tiles(mid, j):
    """k_block_dot<4> on its 128 x 4 grid: 302 tiles per field, so every workgroup takes a second and a third."""
    run_block_dot(mid, j, 4, 128)


@pytest.mark.parametrize("j", [1, 5])
def test_block_dot_large_tiles(big, j):
    """k_block_dot<8> (256 x 4 grid, 938 tiles per field) against numpy, not against another driver."""
    run_block_dot(big, j, 8, 256)


# ---- block update: accumulate + norm, overwrite --------------------------------------------------------------------
def run_block_update(e, j, pairs, grid, launches, last_grid=None, stride=True):
    lay, ctx = e.lay, e.ctx
    p = stream_plan(lay, "block_update", j, NKV_NORM2)
    assert (p.kernel, p.pairs, p.grid_x, p.launches) == ("block_update", pairs, grid, launches), dict(p)
    assert p == stream_plan(lay, "block_update", j, NKV_NORM2 | NKV_OVERWRITE)
    if launches > 1:
        assert p.launches >= 2 and p.last_grid_x == last_grid < p.grid_x and p.band_tiles == 2 * p.grid_x, dict(p)
    elif stride:
        assert p.tiles > p.grid_x, dict(p)
    else:
        assert p.tiles == p.grid_x, dict(p)
    print(f"block_update j={j}: k_block_update<*,*,{p.pairs}>, {p.tiles} tiles, {p.launches} launch(es) of "
          f"{p.band_tiles} tiles on {p.grid_x} workgroups, the last on {p.last_grid_x}")
    h = coeffs(j)
    hd = e.upload(h)
    nrm = torch.full((2,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(j):
        ctx.call("nkv_block_update", ctx.w.data_ptr(), e.Q.ptr, j, hd.data_ptr(), e.f.ptr, nrm.data_ptr(),
                 ctx.ws.data_ptr(), NKV_NORM2 | NKV_TIME, ctx.stream)
        got, nr = e.f.to_packed(), nrm.cpu().numpy()
    fref = ref_update(e, j, h, e.fh)
    # the time slot: updated exactly once whatever the number of bands
    check_vector(lay, got, fref[:lay.rows], e.fh, time_want=fref[lay.time_offset])
    np.testing.assert_allclose(nr[0], ref_norm(e, fref), rtol=1e-12)     # every band's share of every partial slot
    assert nr[1] == -3.0
    # overwrite (k_matmul): out = Q h over a vector that held other data, time included; then without NKV_TIME
    for flags in (NKV_OVERWRITE | NKV_TIME, NKV_OVERWRITE):
        with e.poisoned(j):
            ctx.call("nkv_block_update", ctx.w.data_ptr(), e.Q.ptr, j, hd.data_ptr(), e.g.ptr, None, ctx.ws.data_ptr(),
                     flags, ctx.stream)
            got = e.g.to_packed()
        want = h @ e.Qh[:j]
        check_vector(lay, got, want[:lay.rows], e.gh, time_want=want[lay.time_offset] if flags & NKV_TIME else None)


@pytest.mark.parametrize("j,grid", [(2, 1336), (5, 1024)])
def test_block_update_small_tiles(mid, j, grid):
    """k_block_update<*, *, 4>: one tile per workgroup on the 4x grid (j = 2), a second trip for 312 workgroups of the
    1024 grid (j = 5)."""
    run_block_update(mid, j, 4, grid, 1, stride=j > 2)


def test_block_update_large_tiles_second_trip(big):
    """k_block_update<*, *, 8>, j = 2: the 4096 grid, one launch, 52 workgroups take a second tile."""
    run_block_update(big, 2, 8, 4096, 1)


def test_block_update_large_tiles_row_bands(big):
    """j = 5: bands of 2048 + 2048 + 52 tiles on 1024, 1024 and 52 workgroups: t_lo > 0, later bands add to the
    partial slots the first band wrote (the last band to 52 of them), the time slot is updated in band 0 only."""
    run_block_update(big, 5, 8, 1024, 3, last_grid=52)


# ---- two-vector dot ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_last", [False, True])
@pytest.mark.parametrize("j", [2, 7])
def test_block_dot2_grid_stride_small_tiles(mid, j, x_last):
    """k_block_dot2<4>, 128 x 4 grid over 302 tiles per field; x a separate vector, or column j-1 (its two dots
    from registers, the column not streamed again)."""
    e, lay, ctx = mid, MID, mid.ctx
    p = stream_plan(lay, "block_dot2", j, NKV_X_IS_LAST if x_last else 0)
    assert (p.kernel, p.pairs, p.grid_x, p.grid_y, p.fields_per_block, p.launches) == ("block_dot2", 4, 128, 4, 1, 1), dict(p)
    assert p.tiles > p.grid_x, dict(p)
    print(f"block_dot2 j={j} x_last={x_last}: k_block_dot2<4>, {p.tiles} tiles per field over 128 x 4 workgroups")
    hout = torch.full((2 * j + 1,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(j):
        xp = e.Q.col_ptr(j - 1) if x_last else e.g.ptr
        ctx.call("nkv_block_dot2", ctx.w.data_ptr(), e.Q.ptr, j, xp, e.f.ptr, hout.data_ptr(), ctx.ws.data_ptr(),
                 NKV_TIME | (NKV_X_IS_LAST if x_last else 0), ctx.stream)
        ho = hout.cpu().numpy()
        assert torch.equal(e.f.storage.view(torch.int64), e.f0.view(torch.int64))
        assert torch.equal(e.g.storage.view(torch.int64), e.g0.view(torch.int64))
    xh = e.Qh[j - 1] if x_last else e.gh
    check_dots(ho[: 2 * j], np.concatenate([ref_dot(e, j, xh, True), ref_dot(e, j, e.fh, True)]))
    assert ho[2 * j] == -3.0


# ---- MGS column step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_qb", [True, False])
def test_axpy_dot_grid_stride(mid, with_qb):
    """k_axpy_dot<4>: 1336 tiles over 1024 workgroups; the dot against the next column, or ||f_new||^2."""
    e, lay, ctx = mid, MID, mid.ctx
    p = stream_plan(lay, "axpy_dot")
    assert (p.kernel, p.pairs, p.grid_x, p.tiles, p.launches) == ("axpy_dot", 4, 1024, 1336, 1), dict(p)
    assert p.tiles > p.grid_x
    print(f"axpy_dot qb={'column 1' if with_qb else 'NULL'}: k_axpy_dot<4>, {p.tiles} tiles over {p.grid_x} workgroups")
    alpha = 0.37
    ad = e.upload([alpha])
    out = torch.full((2,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(2):
        ctx.call("nkv_axpy_dot", ctx.w.data_ptr(), e.f.ptr, ad.data_ptr(), e.Q.col_ptr(0), e.Q.col_ptr(1) if with_qb else None,
                 out.data_ptr(), ctx.ws.data_ptr(), NKV_TIME | NKV_TIME_DOT, ctx.stream)
        got, o = e.f.to_packed(), out.cpu().numpy()
    fref = e.fh - alpha * e.Qh[0]
    t = lay.time_offset
    check_vector(lay, got, fref[:lay.rows], e.fh, time_want=fref[t])
    b = e.Qh[1] if with_qb else fref
    ref = np.sum(e.wf * fref * b) + fref[t] * b[t]
    np.testing.assert_allclose(o[0], ref, rtol=1e-12, atol=1e-12 * abs(ref))
    assert o[1] == -3.0


# ---- DCGS2 dual update -----------------------------------------------------------------------------------------------
def run_dcgs2_update(e, m, with_norm, pairs, launches, loop, units):
    lay, ctx = e.lay, e.ctx
    p = stream_plan(lay, "dcgs2_update", m, NKV_NORM2 if with_norm else 0)
    assert (p.kernel, p.pairs, p.grid_x, p.launches, p.work_loop, p.units) == ("dcgs2_update", pairs, 768, launches, loop,
                                                                             units), dict(p)
    if launches > 1:
        assert p.launches >= 2 and p.band_tiles == 2 * p.grid_x and p.tiles - (launches - 1) * p.band_tiles > 0, dict(p)
    assert p.units > p.grid_x, dict(p)
    print(f"dcgs2_update m={m} norm={with_norm}: k_dcgs2_update<{p.pairs},{str(with_norm).lower()}>, {p.work_loop} loop, "
          f"{p.units} units over {p.grid_x} workgroups, {p.launches} launch(es) of {p.band_tiles} tiles")
    coef, a, x, rinv, yc, sc = dcgs2_coef(m)
    ctx.coef[: coef.size].copy_(torch.as_tensor(coef))
    nrm = torch.full((2,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(m + 1, written=(m,)):
        e.out.storage.copy_(e.g0)        # fout held other data: every row of it is written
        ctx.call("nkv_dcgs2_update", ctx.w.data_ptr(), e.Q.ptr, m, ctx.coef.data_ptr(), e.Q.col_ptr(m), e.f.ptr, e.out.ptr,
                 nrm.data_ptr() if with_norm else None, ctx.ws.data_ptr(), NKV_TIME, ctx.stream)
        qgot, fgot, nr = e.Q.storage[m].cpu().numpy(), e.out.to_packed(), nrm.cpu().numpy()
        assert torch.equal(e.f.storage.view(torch.int64), e.f0.view(torch.int64))      # the matvec output is only read
    t = lay.time_offset
    qbar = (e.Qh[m] * sc - a @ e.Qh[:m]) * rinv
    fref = e.fh * (sc * rinv) - x @ e.Qh[:m] - qbar * yc
    check_vector(lay, qgot, qbar[:lay.rows], e.Qh[m], time_want=qbar[t])
    check_vector(lay, fgot, fref[:lay.rows], e.gh, time_want=fref[t])
    if with_norm:
        np.testing.assert_allclose(nr[0], ref_norm(e, fref), rtol=1e-12)
    else:
        assert nr[0] == -3.0   # no norm requested: nothing reduced, nothing written
    assert nr[1] == -3.0


@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("m", [0, 1, 9])
def test_dcgs2_update_large_tiles(big, m, with_norm):
    """Without norm: bands of 1536 + 1536 + 1076 tiles (t_lo > 0, t_hi < tiles).  With norm: the per-unit loop (one
    row tile of each of the four fields per trip, then the 396 pressure tiles), 1334 units over 768 workgroups, at
    m below and above the m >= 8 rule (m = 9: four pairs of columns and an odd one)."""
    if with_norm:
        run_dcgs2_update(big, m, True, 8, 1, "units", 938 + 396)
    else:
        run_dcgs2_update(big, m, False, 8, 3, "tiles", 4148)


def test_dcgs2_update_per_tile_norm_loop_with_stride(mid):
    """k_dcgs2_update<4, true> at m = 9 with 302 < 768 tiles per field: the per-tile loop, 1336 tiles over 768
    workgroups (the weight row of a second-trip tile comes from t / tiles_per_field)."""
    run_dcgs2_update(mid, 9, True, 4, 1, "tiles", 1336)


# ---- BLAS-1 and the finish kernel on their grid-stride loops --------------------------------------------------------
def run_blas1(e, op):
    lay, ctx = e.lay, e.ctx
    rows, t = lay.rows, lay.time_offset
    fh, gh, q0 = e.fh, e.gh, e.Qh[0]
    x, y, z = e.f, e.g, e.out
    if op == "axpby":
        # axpby: time untouched without NKV_TIME; x*a + y*b uncontracted on the host, contracted on the device
        ctx.call("nkv_axpby", x.ptr, 0.7, y.ptr, -1.3, 0, ctx.stream)
        check_vector(lay, x.to_packed(), fh[:rows] * 0.7 + gh[:rows] * -1.3, fh, atol=4e-16 * 3, rtol=0)
        # ... in place (y is x) and with the time slot
        e.reset()
        ctx.call("nkv_axpby", x.ptr, 0.7, x.ptr, -1.3, NKV_TIME, ctx.stream)
        check_vector(lay, x.to_packed(), fh[:rows] * 0.7 + fh[:rows] * -1.3, fh, time_want=F_TIME * 0.7 + F_TIME * -1.3,
                     atol=4e-16 * 3, rtol=0)
    elif op == "scal":
        # scal, with and without time
        ctx.call("nkv_scal", x.ptr, -2.5, NKV_TIME, ctx.stream)
        check_vector(lay, x.to_packed(), fh[:rows] * -2.5, fh, time_want=F_TIME * -2.5, exact=True)
        ctx.call("nkv_scal", y.ptr, 3.0, 0, ctx.stream)
        check_vector(lay, y.to_packed(), gh[:rows] * 3.0, gh, exact=True)
    elif op == "copy_zero":
        # copy over other data, from a basis column; zero
        ctx.call("nkv_copy", x.ptr, e.Q.col_ptr(0), NKV_TIME, ctx.stream)
        check_vector(lay, x.to_packed(), q0[:rows], fh, time_want=q0[t], exact=True)
        ctx.call("nkv_copy", y.ptr, e.Q.col_ptr(0), 0, ctx.stream)
        check_vector(lay, y.to_packed(), q0[:rows], gh, exact=True)
        ctx.call("nkv_zero", x.ptr, NKV_TIME, ctx.stream)
        assert not x.to_packed().any()
        e.reset()
        ctx.call("nkv_zero", x.ptr, 0, ctx.stream)
        got = x.to_packed()
        assert not got[:rows].any()
        assert_same_bits(got[rows:], fh[rows:])
    elif op == "sub3":
        # sub3: three vectors, then p aliasing q, then p aliasing r
        z.storage.copy_(e.Q0[0])
        ctx.call("nkv_sub3", z.ptr, x.ptr, y.ptr, NKV_TIME, ctx.stream)
        check_vector(lay, z.to_packed(), fh[:rows] - gh[:rows], q0, time_want=F_TIME - G_TIME, exact=True)
        ctx.call("nkv_sub3", x.ptr, x.ptr, y.ptr, NKV_TIME, ctx.stream)
        check_vector(lay, x.to_packed(), fh[:rows] - gh[:rows], fh, time_want=F_TIME - G_TIME, exact=True)
        e.reset()
        ctx.call("nkv_sub3", y.ptr, x.ptr, y.ptr, 0, ctx.stream)
        check_vector(lay, y.to_packed(), fh[:rows] - gh[:rows], gh, exact=True)
    else:
        # axpy_dev: x + sign * (*alpha_dev) * y, the product formed first, then one FMA per row
        ad = e.upload([0.37])
        ctx.call("nkv_axpy_dev", x.ptr, ad.data_ptr(), -1.0, y.ptr, NKV_TIME, ctx.stream)
        check_vector(lay, x.to_packed(), fh[:rows] + (-1.0 * 0.37) * gh[:rows], fh, time_want=F_TIME - 0.37 * G_TIME)
        e.reset()
        ctx.call("nkv_axpy_dev", x.ptr, ad.data_ptr(), 1.0, x.ptr, 0, ctx.stream)       # y is x
        check_vector(lay, x.to_packed(), fh[:rows] + 0.37 * fh[:rows], fh)
        assert torch.equal(y.storage.view(torch.int64), e.g0.view(torch.int64))


@pytest.mark.parametrize("op", ["axpby", "scal", "copy_zero", "sub3", "axpy_dev"])
def test_blas1_grid_stride(big, op):
    """k_blas1<*>: 8296 chunks over 4096 workgroups.  The assertions of test_blas1_vs_oracle: copy, zero, scal and
    sub3 bit-exact, axpby within 3 ulp of 2; in place where the kernel allows aliasing."""
    p = stream_plan(BIG, "blas1")
    assert (p.kernel, p.tiles, p.grid_x, p.launches, p.rows_per_tile) == ("blas1", 8296, 4096, 1, 2048), dict(p)
    assert p.tiles > p.grid_x
    print(f"blas1 {op}: k_blas1<*>, {p.tiles} chunks over {p.grid_x} workgroups")
    with big.poisoned(1):
        run_blas1(big, op)


def test_finish_grid_stride(big):
    """k_finish: 8296 chunks over 4096 workgroups, in place (nkv_normalize_dev), into another vector
    (nkv_normalize_store) and with the H column (nkv_arnoldi_finish).  nrm2 = 6.25: beta = 2.5 exactly, and one
    correctly rounded 1 / beta, so q = f * (1 / 2.5) holds bit for bit, the time slot included."""
    e, lay, ctx = big, BIG, big.ctx
    p = stream_plan(lay, "finish")
    assert (p.kernel, p.tiles, p.grid_x, p.launches, p.rows_per_tile) == ("finish", 8296, 4096, 1, 2048), dict(p)
    assert p.tiles > p.grid_x
    print(f"finish: k_finish, {p.tiles} chunks over {p.grid_x} workgroups")
    rows = lay.rows
    inv = 1.0 / 2.5
    nrm2, beta = e.upload([6.25]), torch.full((2,), -3.0, dtype=torch.float64, device=ctx.device)
    with e.poisoned(1, written=(0,)):
        ctx.call("nkv_normalize_dev", e.f.ptr, nrm2.data_ptr(), beta.data_ptr(), 0, ctx.stream)
        check_vector(lay, e.f.to_packed(), e.fh[:rows] * inv, e.fh, time_want=F_TIME * inv, exact=True)
        assert beta.cpu().tolist() == [2.5, -3.0]
        beta.fill_(-3.0)
        ctx.call("nkv_normalize_store", e.g.ptr, nrm2.data_ptr(), e.out.ptr, beta.data_ptr(), 0, ctx.stream)
        check_vector(lay, e.out.to_packed(), e.gh[:rows] * inv, np.zeros(lay.ld), time_want=G_TIME * inv, exact=True)
        assert beta.cpu().tolist() == [2.5, -3.0]
        assert torch.equal(e.g.storage.view(torch.int64), e.g0.view(torch.int64))
        j = 5
        h1, h2 = e.upload(coeffs(j)), e.upload(coeffs(j)[::-1] * 1e-3)
        hcol = torch.full((j + 2,), -3.0, dtype=torch.float64, device=ctx.device)
        ctx.call("nkv_arnoldi_finish", e.g.ptr, nrm2.data_ptr(), e.Q.col_ptr(0), j, h1.data_ptr(), h2.data_ptr(),
                 hcol.data_ptr(), 0, ctx.stream)
        check_vector(lay, e.Q.storage[0].cpu().numpy(), e.gh[:rows] * inv, e.Qh[0], time_want=G_TIME * inv, exact=True)
        assert_same_bits(hcol.cpu().numpy(), np.concatenate([coeffs(j) + coeffs(j)[::-1] * 1e-3, [2.5, -3.0]]))


# ---- the launchers refuse what the plan refuses --------------------------------------------------------------------
def test_plan_and_launchers_refuse_alike(fuse):
    e, ctx = fuse, fuse.ctx
    e.reset()
    lib, Lp = _lib.load(), ctypes.byref(ctx.L)
    w, Q, f, h, ws, s = ctx.w.data_ptr(), e.Q.ptr, e.f.ptr, ctx.h1.data_ptr(), ctx.ws.data_ptr(), ctx.stream
    plan = _lib.nkv_plan()
    calls = [
        (_lib.NKV_STREAM_BLOCK_DOT, 0, lambda j: lib.nkv_block_dot(Lp, w, Q, j, f, h, ws, 0, s)),
        (_lib.NKV_STREAM_BLOCK_DOT, _lib.NKV_MAX_COLS + 1, lambda j: lib.nkv_block_dot(Lp, w, Q, j, f, h, ws, 0, s)),
        (_lib.NKV_STREAM_BLOCK_UPDATE, -1, lambda j: lib.nkv_block_update(Lp, w, Q, j, h, f, None, ws, 0, s)),
        (_lib.NKV_STREAM_UPDATE_DOT, 0, lambda j: lib.nkv_block_update_dot(Lp, w, Q, j, h, f, h, ws, 0, s)),
        (_lib.NKV_STREAM_UPDATE_DOT, _lib.NKV_MAX_COLS + 1, lambda j: lib.nkv_block_update_dot(Lp, w, Q, j, h, f, h, ws, 0, s)),
        (_lib.NKV_STREAM_BLOCK_DOT2, 0, lambda j: lib.nkv_block_dot2(Lp, w, Q, j, f, f, h, ws, 0, s)),
        (_lib.NKV_STREAM_DCGS2_UPDATE, -1, lambda j: lib.nkv_dcgs2_update(Lp, w, Q, j, h, f, f, e.g.ptr, None, ws, 0, s)),
    ]
    for op, j, launcher in calls:
        want = lib.nkv_stream_plan(Lp, op, j, 0, ctypes.byref(plan))
        msg = _lib.last_error()
        assert want != _lib.NKV_OK
        assert launcher(j) == want
        assert _lib.last_error() == msg
    assert torch.equal(e.f.storage.view(torch.int64), e.f0.view(torch.int64))
