"""The launch shapes of the streaming entry points (nkv_stream_plan, csrc/core.hip) against an independent
restatement of their rules: pairs per thread, grid, row bands, the work loop of the DCGS2 update, the partial
slots.  Host only: the layouts are plain structs, nothing is allocated and no GPU is needed.

The launchers of csrc/vector.hip, csrc/gram_schmidt.hip and nkv_op_diag decide through nkv_stream_plan, so a
changed knob (NKV_SMALL_TILES, NKV_MAXB, NKV_DC_G, NKV_UPD_ROUNDS, NKV_DC_ROUNDS, NKV_FUSE_G, NKV_FUSE_G_MID,
NKV_DOT_SMALL_B, NKV_D2_MAXB, NKV_UPD_SMALL_J, ...) fails here before it silently moves the cases of
tests/test_gpu_stream_paths.py to another loop shape."""
import ctypes

import numpy as np
import pytest

from nekstab_next_amd import _lib
from nekstab_next_amd._lib import NKV_EINVAL, NKV_ESHAPE, NKV_MAX_COLS, NKV_NORM2, NKV_OK, NKV_OVERWRITE, NKV_TILE, NKV_X_IS_LAST
from nekstab_next_amd.layout import NekLayout, box3d_layout
from nekstab_next_amd.vector import STREAM_OPS, stream_plan

WG = 256                      # threads per workgroup of every kernel but the fused pass
SMALL = NekLayout(ldim=3, lx1=5, lx2=3, nelgv=37, n_scalars=1)   # LAYOUTS["3d_scalar"] of the GPU suite
BOX70, BOX1203, BOX7501 = box3d_layout(70), box3d_layout(1203), box3d_layout(7501)
OPTIONAL = NekLayout(ldim=2, lx1=8, lx2=6, nelgv=48001)


def struct(n_wf, field_tiles, pr_tiles=0):
    """n_wf weighted fields of field_tiles NKV_TILE-row tiles and a pressure segment of pr_tiles: passes
    check_layout, allocates nothing."""
    sv, sp = field_tiles * NKV_TILE, pr_tiles * NKV_TILE
    return _lib.nkv_layout(n_v=sv, n_p=sp, sv=sv, sp=sp, ld=n_wf * sv + sp + NKV_TILE, n_wf=n_wf, rank0=1)


def rows_of(L):
    return L.n_wf * L.sv + L.sp


def bands(n, grid, rounds, shrink=True):
    """Row bands of `rounds` grid-stride rounds once the loop holds two of them; the launches as (lo, hi, grid):
    the first has the whole grid (every partial slot is written before a band adds to it), the last no more
    workgroups than items."""
    band = rounds * grid if rounds > 0 and n >= 2 * rounds * grid else max(n, 1)
    out = []
    for lo in range(0, max(n, 1), band):
        hi = min(lo + band, n)
        out.append((lo, hi, grid if lo == 0 or not shrink else min(grid, hi - lo)))
    return band, out


def expected(L, op, j=1, flags=0):
    """The rule, restated from what the kernels need (not from the dispatch code)."""
    rows = rows_of(L)
    large = rows // 4096 >= 2048          # enough 8-pair tiles to fill the chip twice over
    e = dict(kernel=op, nw=0, cpw=0, wg_threads=WG, grid_y=1, work_loop="tiles", fields_per_block=1,
             partial_slots=0, partial_cols=0)
    rounds = 0
    if op in ("block_dot", "block_dot2"):
        two = op == "block_dot2"
        e["pairs"] = 8 if large else 4
        tile = WG * 2 * e["pairs"]
        e["tiles"] = L.sv // tile                                    # per weighted field
        e["fields_per_block"] = L.n_wf if two and large else 1       # the block's own field loop
        e["grid_y"] = L.n_wf // e["fields_per_block"]
        cap = (256 if large else 512) if two else (1024 if large else 512)
        e["grid_x"] = max(1, min(cap // e["grid_y"], e["tiles"]))
        e["partial_slots"] = e["grid_x"] * e["grid_y"] if e["tiles"] else 0
        e["partial_cols"] = 2 * j if two else j
        e["units"] = e["tiles"]
        e["band_tiles"], e["launches"], e["last_grid_x"] = max(e["tiles"], 1), 1 if e["tiles"] else 0, e["grid_x"]
        e["rows_per_tile"] = tile
        return e
    if op == "update_dot":
        if j > 256 or rows >= 2 ** 29:
            return dict(kernel="split")
        e["nw"] = 4 if j <= 12 else 8 if j <= 128 else 16
        e["cpw"] = -(-j // e["nw"])
        e["pairs"], e["wg_threads"], tile = 1, 64 * e["nw"], 128
        cap = 512 if 16 <= j <= 32 else 1024
        e["partial_cols"] = j
    elif op == "block_update":
        e["pairs"] = 8 if large else 4
        tile = WG * 2 * e["pairs"]
        cap, rounds = (4096 if j <= 2 else 1024), 2
        e["partial_cols"] = 1 if flags & NKV_NORM2 else 0
    elif op == "dcgs2_update":
        e["pairs"] = 8 if large else 4
        tile = WG * 2 * e["pairs"]
        cap, rounds = 768, 0 if flags & NKV_NORM2 else 2
        e["partial_cols"] = 1 if flags & NKV_NORM2 else 0
    elif op == "axpy_dot":
        e["pairs"], tile, cap = 4, WG * 2 * 4, 1024
        e["partial_cols"] = 1
    else:                                   # blas1 / finish / op_diag: chunks of 4 double2 per thread
        e["pairs"], tile = 4, WG * 2 * 4
        cap = None
        rounds = 2 if op == "op_diag" else 0
    e["rows_per_tile"] = tile
    e["tiles"] = e["units"] = rows // tile
    if cap is None:                         # one thread per row pair (BLAS-1: and the time slot's), 4096 at the most
        pairs = rows // 2 + (1 if op == "blas1" else 0)
        e["grid_x"] = max(1, min(-(-pairs // WG), 4096))
    else:
        e["grid_x"] = max(1, min(e["tiles"], cap))
    e["band_tiles"], launches = bands(e["tiles"], e["grid_x"], rounds, shrink=op != "op_diag")
    e["launches"], e["last_grid_x"] = len(launches), launches[-1][2]
    if e["partial_cols"]:
        e["partial_slots"] = e["grid_x"] if (e["tiles"] or op != "axpy_dot") else 0
    if op == "dcgs2_update" and flags & NKV_NORM2:
        tpf = L.sv // tile
        if not (tpf < e["grid_x"] and j >= 8):    # a row tile of every field per trip, then the pressure tiles
            e["work_loop"], e["units"] = "units", tpf + (e["tiles"] - tpf * L.n_wf)
    return e


def check(L, op, j=1, flags=0):
    L = L.c_struct() if isinstance(L, NekLayout) else L
    got, want = stream_plan(L, op, j, flags), expected(L, op, j, flags)
    if want["kernel"] == "split":
        assert got.kernel == "split" and not any(v for k, v in got.items() if k not in ("kernel", "work_loop"))
        return got
    assert dict(got) == want, (op, j, flags, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    return got


OPS_J = [("block_dot", (1, 4, 5, 37, 1024)), ("block_update", (0, 1, 2, 3, 5, 64)),
         ("update_dot", (1, 2, 12, 13, 15, 16, 32, 33, 64, 100, 128, 129, 200, 256, 257, 1024)),
         ("block_dot2", (1, 2, 7, 33, 1024)), ("dcgs2_update", (0, 1, 7, 8, 9, 31)), ("axpy_dot", (1,)), ("blas1", (1,)),
         ("finish", (1,)), ("op_diag", (1,))]
FLAGS = {"block_update": (0, NKV_NORM2, NKV_OVERWRITE, NKV_NORM2 | NKV_OVERWRITE), "dcgs2_update": (0, NKV_NORM2),
         "block_dot2": (0, NKV_X_IS_LAST)}
TEST_LAYOUTS = [SMALL, NekLayout(ldim=2, lx1=6, lx2=4, nelgv=300), BOX70, box3d_layout(120), BOX1203, box3d_layout(4000),
                NekLayout(ldim=3, lx1=8, lx2=6, nelgv=6000, ifpo=False), BOX7501, OPTIONAL]


def test_every_op_on_the_suites_layouts():
    """Every op, its column counts on both sides of each column rule (2|3, 12|13, 15|16, 32|33, 128|129, 256|257,
    7|8) and every shape flag, on the layouts the GPU suites use."""
    n = 0
    for lay in TEST_LAYOUTS:
        for op, js in OPS_J:
            for j in js:
                for fl in FLAGS.get(op, (0,)):
                    check(lay, op, j, fl)
                    n += 1
    assert n > 400


def test_small_large_flip_at_2048_large_tiles():
    lo, hi = struct(1, 2047), struct(1, 2048)
    for op in ("block_dot", "block_update", "block_dot2", "dcgs2_update"):
        a, b = check(lo, op, 5), check(hi, op, 5)
        assert (a.pairs, a.rows_per_tile, b.pairs, b.rows_per_tile) == (4, 2048, 8, 4096), op
    assert check(lo, "axpy_dot").pairs == check(hi, "axpy_dot").pairs == 4      # one instantiation at every size
    a, b = check(lo, "block_dot", 5), check(hi, "block_dot", 5)
    assert (a.grid_x, b.grid_x) == (512, 1024)
    lo4, hi4 = struct(4, 511, 3), struct(4, 511, 4)                          # the pressure tiles count too
    a, b = check(lo4, "block_dot2", 5), check(hi4, "block_dot2", 5)
    assert (a.grid_x, a.grid_y, a.fields_per_block) == (128, 4, 1) and (b.grid_x, b.grid_y, b.fields_per_block) == (256, 1, 4)


def test_update_bands_start_at_two_bands():
    """tiles >= 2 * 2 * grid: 4096 tiles of the 1024 grid (j >= 3), 16384 of the 4096 grid (j <= 2)."""
    for j, t in ((3, 4096), (5, 4096), (2, 16384), (0, 16384)):
        a, b = check(struct(1, t - 1), "block_update", j, NKV_NORM2), check(struct(1, t), "block_update", j, NKV_NORM2)
        g = t // 4
        assert (a.launches, a.band_tiles, a.grid_x) == (1, t - 1, g), (j, dict(a))
        assert (b.launches, b.band_tiles, b.grid_x, b.last_grid_x) == (2, 2 * g, g, g), (j, dict(b))
    p = check(struct(1, 4097), "block_update", 3)
    assert (p.launches, p.last_grid_x) == (3, 1)
    assert (check(struct(1, 3), "block_update", 2).grid_x, check(struct(1, 3), "block_update", 3).grid_x) == (6, 6)
    assert (check(struct(1, 2100), "block_update", 2).grid_x, check(struct(1, 2100), "block_update", 3).grid_x) == (2100, 1024)


def test_dcgs2_bands_and_norm_loop():
    """Without norm: bands from 3072 tiles of the 768 grid (small tiles come in pairs: 3070 | 3072).  With norm: one
    launch; the per-tile loop iff a field has fewer tiles than the grid AND m >= 8."""
    for lo, hi in ((struct(1, 3071), struct(1, 3072)), (struct(1, 1535), struct(1, 1536))):
        a, b = check(lo, "dcgs2_update", 9), check(hi, "dcgs2_update", 9)
        assert (a.launches, a.grid_x) == (1, 768) and (b.launches, b.band_tiles, b.last_grid_x) == (2, 1536, 768)
        assert check(hi, "dcgs2_update", 9, NKV_NORM2).launches == 1
    assert check(struct(1, 1535), "dcgs2_update", 9).pairs == 4 and check(struct(1, 3071), "dcgs2_update", 9).pairs == 8
    p = check(struct(1, 3073), "dcgs2_update", 0)
    assert (p.launches, p.last_grid_x) == (3, 1)
    f767, f768 = struct(3, 767, 5), struct(3, 768, 5)
    for m, loop767 in ((7, "units"), (8, "tiles"), (9, "tiles"), (0, "units")):
        a, b = check(f767, "dcgs2_update", m, NKV_NORM2), check(f768, "dcgs2_update", m, NKV_NORM2)
        assert (a.work_loop, b.work_loop) == (loop767, "units"), m
        assert b.units == 768 + 5 and a.units == (767 + 5 if loop767 == "units" else 3 * 767 + 5)
        assert check(f767, "dcgs2_update", m).work_loop == "tiles"


def test_op_diag_bands_and_stream_grids():
    a, b = check(struct(1, 8191), "op_diag"), check(struct(1, 8192), "op_diag")     # 16382 | 16384 chunks
    assert (a.launches, a.tiles) == (1, 16382) and (b.launches, b.band_tiles, b.grid_x, b.last_grid_x) == (2, 8192, 4096, 4096)
    p = check(struct(1, 8193), "op_diag")
    assert (p.launches, p.last_grid_x) == (3, 4096)                                   # op_diag keeps its grid
    for op in ("blas1", "finish"):
        assert check(struct(1, 8192), op).launches == 1
    assert (check(struct(1, 3), "blas1").grid_x, check(struct(1, 3), "finish").grid_x) == (25, 24)
    assert (check(struct(1, 512), "blas1").grid_x, check(struct(1, 511), "blas1").grid_x) == (4096, 4089)


def test_fused_pass_instantiations():
    """k_update_dot<NW, CPW>: 4 waves to j = 12, 8 to 128, 16 to 256, then the two-pass fallback; the 512 grid for
    16 <= j <= 32; one launch whatever the size (NKV_FUSE_ROUNDS = 0)."""
    want = {2: (4, 1, 1024), 12: (4, 3, 1024), 13: (8, 2, 1024), 15: (8, 2, 1024), 16: (8, 2, 512), 32: (8, 4, 512),
            33: (8, 5, 1024), 64: (8, 8, 1024), 100: (8, 13, 1024), 128: (8, 16, 1024), 129: (16, 9, 1024),
            200: (16, 13, 1024), 256: (16, 16, 1024)}
    for j, (nw, cpw, g) in want.items():
        p = check(BOX70, "update_dot", j)
        assert (p.nw, p.cpw, p.grid_x, p.wg_threads, p.rows_per_tile, p.tiles, p.launches) == (nw, cpw, g, 64 * nw, 128, 1280, 1)
        assert check(BOX7501, "update_dot", j).launches == 1
    assert check(BOX70, "update_dot", 257).kernel == "split"
    assert check(struct(1, 2 ** 17 - 1), "update_dot", 5).kernel == "update_dot"      # rows < 2^29: 32-bit offsets
    assert check(struct(1, 2 ** 17), "update_dot", 5).kernel == "split"
    assert check(BOX7501, "axpy_dot").launches == 1                                     # NKV_AXD_ROUNDS = 0


def test_the_layouts_of_the_gpu_paths_module():
    """The table of tests/test_gpu_stream_paths.py's docstring."""
    assert (BOX70.rows, BOX1203.rows, BOX7501.rows, OPTIONAL.rows) == (163_840, 2_736_128, 16_990_208, 7_880_704)
    p = check(BOX1203, "block_dot", 5)
    assert (p.pairs, p.tiles, p.grid_x, p.grid_y) == (4, 302, 128, 4)
    p = check(BOX1203, "dcgs2_update", 9, NKV_NORM2)
    assert (p.pairs, p.work_loop, p.units, p.grid_x) == (4, "tiles", 1336, 768)
    p = check(BOX7501, "block_update", 5, NKV_NORM2)
    assert (p.pairs, p.tiles, p.launches, p.band_tiles, p.grid_x, p.last_grid_x) == (8, 4148, 3, 2048, 1024, 52)
    p = check(BOX7501, "block_update", 2, NKV_NORM2)
    assert (p.launches, p.grid_x, p.tiles) == (1, 4096, 4148)
    p = check(BOX7501, "dcgs2_update", 9)
    assert (p.launches, p.band_tiles, p.tiles - 2 * p.band_tiles, p.last_grid_x) == (3, 1536, 1076, 768)
    p = check(BOX7501, "dcgs2_update", 9, NKV_NORM2)
    assert (p.work_loop, p.units, p.grid_x) == ("units", 938 + 396, 768)
    assert (check(BOX7501, "blas1").tiles, check(BOX7501, "blas1").grid_x) == (8296, 4096)
    p, q = check(OPTIONAL, "dcgs2_update", 9), check(OPTIONAL, "dcgs2_update", 9, NKV_NORM2)
    assert (p.pairs, p.tiles, p.launches, q.work_loop, q.units) == (4, 3848, 3, "units", 1502 + 844)


def test_empty_shard():
    """A rank without elements: the dots launch only their second stage over no partials; every other entry point
    launches once (the time slot)."""
    L = _lib.nkv_layout(n_v=0, n_p=0, sv=0, sp=0, ld=NKV_TILE, n_wf=3, rank0=0)
    for op, js in OPS_J:
        for fl in FLAGS.get(op, (0,)):
            p = check(L, op, min(js[-1], 5), fl)
            assert p.tiles == 0 and p.grid_x == 1
            assert p.launches == (0 if op in ("block_dot", "block_dot2") else 1), op
            assert p.partial_slots == (1 if op in ("update_dot", "block_update", "dcgs2_update") and p.partial_cols else 0)


def walked(L, p):
    """How often the launches of plan p visit each row tile of the vector (in units of p.rows_per_tile rows)."""
    total = rows_of(L) // p.rows_per_tile
    seen = np.zeros(total, dtype=np.int64)
    tpf = L.sv // p.rows_per_tile
    if p.kernel in ("block_dot", "block_dot2"):                     # weighted fields only
        assert p.grid_y * p.fields_per_block == L.n_wf and p.tiles == tpf
        for bx in range(p.grid_x if p.launches else 0):
            for f in range(L.n_wf):
                seen[f * tpf + np.arange(bx, tpf, p.grid_x)] += 1
        return seen[: L.n_wf * tpf], None
    if p.work_loop == "units":
        assert p.launches == 1
        for b in range(p.grid_x):
            for u in range(b, p.units, p.grid_x):
                if u < tpf:
                    seen[np.arange(L.n_wf) * tpf + u] += 1
                else:
                    seen[L.n_wf * tpf + u - tpf] += 1
        return seen, None
    first_band_blocks = None
    for i in range(p.launches):
        lo, hi = i * p.band_tiles, min((i + 1) * p.band_tiles, p.tiles)
        g = p.last_grid_x if i + 1 == p.launches else p.grid_x
        assert i == 0 or lo < hi
        if i == 0:
            first_band_blocks = g
        assert g <= first_band_blocks                                # a later band adds to slots band 0 wrote
        for b in range(g):
            seen[np.arange(lo + b, hi, g)] += 1
    return seen, first_band_blocks


@pytest.mark.parametrize("lay", [SMALL, BOX70, BOX1203, BOX7501, OPTIONAL, struct(1, 4097), struct(3, 1366, 1),
                                 struct(1, 8193), struct(2, 8200, 3)],
                         ids=["small", "box70", "box1203", "box7501", "optional", "4097", "3x1366+1", "8193", "2x8200+3"])
def test_every_tile_is_walked_exactly_once_and_partials_fit(lay):
    L = lay.c_struct() if isinstance(lay, NekLayout) else lay
    lib = _lib.load()
    for op, js in OPS_J:
        for j in js:
            for fl in FLAGS.get(op, (0,)):
                p = stream_plan(L, op, j, fl)
                if p.kernel == "split":
                    continue
                seen, _ = walked(L, p)
                assert seen.size and (seen == 1).all(), (op, j, fl, dict(p))
                # the slots the kernels write, for the workspace the caller must have sized for these columns
                cols = j if op in ("block_dot", "update_dot", "block_dot2") else 1
                ws = lib.nkv_workspace_bytes(ctypes.byref(L), cols)
                slots = max(p.grid_x * p.grid_y, p.partial_slots) * p.partial_cols
                assert 256 + 8 * slots <= ws, (op, j, fl, slots, ws)
                assert p.partial_slots <= p.grid_x * p.grid_y


# ---- argument errors: the launchers' own checks, from the one place that makes them ------------------
def _raw(L, op, j, flags=0, plan=True):
    p = _lib.nkv_plan()
    p.kernel = -7
    rc = _lib.load().nkv_stream_plan(None if L is None else ctypes.byref(L), op, j, flags, ctypes.byref(p) if plan else None)
    return rc, p.kernel


@pytest.mark.parametrize("op,j,word", [
    ("block_dot", 0, "j=0"), ("block_dot", NKV_MAX_COLS + 1, "j=1025"), ("block_update", -1, "j=-1"),
    ("update_dot", 0, "j=0"), ("update_dot", NKV_MAX_COLS + 1, "j=1025"), ("block_dot2", 0, "j=0"),
    ("block_dot2", NKV_MAX_COLS + 1, "j=1025"), ("dcgs2_update", -1, "m=-1")])
def test_argument_errors(op, j, word):
    """The statuses and messages the launchers give for the same bad column count (tests/test_gpu_stream_paths.py
    asserts that the two agree); the plan is left alone."""
    rc, kernel = _raw(SMALL.c_struct(), STREAM_OPS[op], j)
    assert rc == NKV_EINVAL and kernel == -7
    assert word in _lib.last_error()


def test_null_bad_layout_unknown_op_and_constants():
    import os
    import re

    L = SMALL.c_struct()
    assert _raw(None, 1, 1)[0] == NKV_EINVAL
    bad = SMALL.c_struct()
    bad.ld += 8
    assert _raw(bad, 1, 1)[0] == NKV_ESHAPE
    assert _raw(L, 1, 1, plan=False)[0] == NKV_EINVAL and "NULL" in _lib.last_error()
    for op in (0, 10, 11, -1):                      # NKV_STREAM_SPLIT is a plan's kernel, not an op
        assert _raw(L, op, 1) == (NKV_EINVAL, -7)
        assert "unknown op" in _lib.last_error()
    for op in ("axpy_dot", "blas1", "finish", "op_diag"):     # j is ignored
        assert _raw(L, STREAM_OPS[op], -5)[0] == NKV_OK
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "nekkrylov.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (NKV_STREAM_[A-Z0-9_]+)\s+(\d+)", txt)}
    assert defs == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("NKV_STREAM_")} and len(defs) == 12
    fields = re.search(r"typedef struct nkv_plan \{\s*int64_t ([^;]+);", txt).group(1)
    assert [f.strip() for f in fields.split(",")] == [n for n, _ in _lib.nkv_plan._fields_]
    with pytest.raises(_lib.NkvError) as e:
        stream_plan(SMALL, "block_dot", 0)
    assert e.value.code == NKV_EINVAL
    assert _lib.load().nkv_abi_version() == 3            # an added entry point does not bump the ABI
