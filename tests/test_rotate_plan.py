"""The dispatch of the restart rotation (nkv_rotate_plan, csrc/rotate.hip) against an independent
restatement of its rule: which of k_rotate_few / k_rotate_wide / k_rotate_stream / k_rotate_chunked, and
which template instantiation, nkv_rotate_cols launches for (layout, k, ldv, n_out).  Host only: the layouts
are plain structs, nothing is allocated and no GPU is needed.

nkv_rotate_cols decides through nkv_rotate_plan, so a changed threshold (NKV_ROTF_MAX, NKV_ROTW_MAX_MB,
NKV_ROT_CHUNK_FROM, an LDS formula, a workgroup shape) fails here before it silently moves the GPU suite's
cases to another kernel."""
import ctypes

import pytest

from nekstab_next_amd import _lib
from nekstab_next_amd._lib import NKV_EINVAL, NKV_ESHAPE, NKV_MAX_COLS, NKV_OK, NKV_ROT_MAX_OUT, NKV_TILE
from nekstab_next_amd.layout import NekLayout
from nekstab_next_amd.vector import ROTATE_PATHS, rotate_plan

LDS_BYTES = 160 * 1024          # LDS of one CU (gfx950)
WIDE_MAX_LD = 178_956_960       # the last stride whose largest lane byte offset (3 ld + 30) * 8 fits uint32_t
SMALL = NekLayout(ldim=2, lx1=6, lx2=4, nelgv=300)   # rows = 32768, ld = 36864: LAYOUTS["2d"] of the GPU suite


def layout_with_ld(ld):
    """One weighted field filling all of ld but its last tile: passes check_layout, allocates nothing."""
    assert ld % NKV_TILE == 0 and ld >= 2 * NKV_TILE
    return _lib.nkv_layout(n_v=ld - NKV_TILE, n_p=0, sv=ld - NKV_TILE, sp=0, ld=ld, n_wf=1, rank0=1)


def expected_plan(k, n_out, ld):
    """The rule, restated from the kernels' needs (not from the dispatch code):
    (path, inst, wg_threads, rows_per_tile)."""
    if n_out <= 16:                                   # VALU kernel, one instantiation per kept-column count;
        pairs = 4 if n_out <= 8 else 2                # 256 threads x row pairs x 2 rows
        return "few", n_out, 256, 256 * pairs * 2
    nact = -(-n_out // 16)                            # 16-column MFMA blocks
    kpad = -(-k // 16) * 16                           # wide: batches of 4 k-steps of 4
    cp = -(-(16 * nact) // 32) * 32 + 16              # wide: LDS row stride, 16 (mod 32) doubles
    if nact <= 4 and kpad * cp * 8 <= LDS_BYTES and (3 * ld + 30) * 8 < 2 ** 32:
        return "wide", nact, 8 * 64, 8 * 32           # 8 waves, a 32-row slab each
    kp = ((k + 31) & ~31) + 2                         # stream: LDS column stride, 2 (mod 32) doubles
    if nact < 17 and nact * 16 * kp * 8 <= LDS_BYTES:
        waves = 16 if nact <= 3 else 8                # a 16-row slab per wave
        return "stream", nact, waves * 64, waves * 16
    mb = next(m for m in (2, 4, 8, 12, 16) if nact <= m)
    waves = 8 if mb <= 8 else 4
    return "chunked", mb, waves * 64, waves * 16


@pytest.fixture(scope="module")
def table():
    """The plan of every valid (k, n_out) at the small layout."""
    L = SMALL.c_struct()
    return {(k, n): rotate_plan(L, k, n) for n in range(1, NKV_ROT_MAX_OUT + 1) for k in range(n, NKV_MAX_COLS + 1)}


K_GRID = (16, 17, 32, 33, 64, 65, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 288, 289, 416, 417, 608, 609,
          NKV_MAX_COLS)


def test_dispatch_table_on_the_boundary_grid(table):
    """n_out = 1..NKV_ROT_MAX_OUT against k = n_out and both sides of every k at which an LDS fit flips
    (wide: 256 | 257 at 33-64 kept columns, 416 | 417 at 17-32; stream: 608 | 609, 416 | 417, 288 | 289,
    224 | 225, 192 | 193, 160 | 161, 128 | 129 for 2..8 column blocks) and the largest k."""
    checked = 0
    for n in range(1, NKV_ROT_MAX_OUT + 1):
        for k in sorted({n, *K_GRID}):
            if k < n:
                continue
            assert table[k, n] == expected_plan(k, n, SMALL.ld), (k, n)
            checked += 1
    assert checked > 4000


def test_dispatch_table_everywhere(table):
    """... and every other valid (k, n_out): no boundary the grid does not know of."""
    bad = [(kn, got, expected_plan(*kn, SMALL.ld)) for kn, got in table.items()
           if got != expected_plan(*kn, SMALL.ld)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("k,n_out,path,inst", [
    (256, 64, "wide", 4), (257, 64, "stream", 4), (300, 64, "chunked", 4), (416, 20, "wide", 2),
    (417, 20, "stream", 2), (609, 20, "chunked", 2), (128, 128, "stream", 8), (200, 128, "chunked", 8),
    (300, 150, "chunked", 12), (576, 256, "chunked", 16),
    (16, 16, "few", 16), (17, 17, "wide", 2), (608, 32, "stream", 2), (416, 48, "stream", 3),
    (288, 64, "stream", 4), (224, 80, "stream", 5), (192, 96, "stream", 6), (160, 112, "stream", 7),
    (129, 128, "chunked", 8), (129, 129, "chunked", 12), (193, 193, "chunked", 16), (NKV_MAX_COLS, 256, "chunked", 16),
])
def test_spot_values(table, k, n_out, path, inst):
    """Values worked out by hand from the kernels' LDS formulas."""
    assert table[k, n_out][:2] == (path, inst)


def test_reachable_instantiations(table):
    """With the default knobs the table selects exactly these kernels.  k_rotate_wide<1> and
    k_rotate_stream<1> are compiled and never chosen (n_out <= 16 is k_rotate_few's): only the
    NKV_ROTF_MAX=0 tuning build runs them, and no test of the default build can."""
    reached = {p[:2] for p in table.values()}
    want = ({("few", n) for n in range(1, 17)} | {("wide", m) for m in (2, 3, 4)}
            | {("stream", m) for m in range(2, 9)} | {("chunked", m) for m in (2, 4, 8, 12, 16)})
    assert reached == want
    assert ("wide", 1) not in reached and ("stream", 1) not in reached
    # launch shapes are a function of (path, inst) alone
    shapes = {}
    for p in table.values():
        assert shapes.setdefault(p[:2], p[2:]) == p[2:]
    for (path, inst), (threads, rows) in shapes.items():
        assert threads % 64 == 0 and threads <= 1024 and NKV_TILE % rows == 0, (path, inst)


# ---- the 32-bit lane offset of k_rotate_wide ---------------------------------------------------------
LD_LAST_32 = WIDE_MAX_LD // NKV_TILE * NKV_TILE        # largest valid stride at or below the bound
LD_FIRST_64 = LD_LAST_32 + NKV_TILE                    # smallest valid stride above it


def test_wide_gate_arithmetic():
    """(3 ld + 30) * 8 is the byte offset of lane 63 (lk = 3, lr = 15) from its wave's row base."""
    assert (3 * WIDE_MAX_LD + 30) * 8 < 2 ** 32 <= (3 * (WIDE_MAX_LD + 1) + 30) * 8
    assert LD_LAST_32 <= WIDE_MAX_LD < LD_FIRST_64
    assert (3 * LD_LAST_32 + 30) * 8 < 2 ** 32 <= (3 * LD_FIRST_64 + 30) * 8


def test_wide_is_not_planned_once_its_lane_offset_would_wrap():
    """ld <= 178,956,960 doubles keeps k_rotate_wide; the next valid stride goes to a 64-bit kernel.  The
    wrap itself (wrong rows read, no error) needs a basis of more than 24 GB and is not run anywhere."""
    lo, hi = layout_with_ld(LD_LAST_32), layout_with_ld(LD_FIRST_64)
    assert rotate_plan(lo, 128, 25) == ("wide", 2, 512, 256)
    assert rotate_plan(hi, 128, 25) == ("stream", 2, 1024, 256)
    # every plan that is wide below the bound is stream or chunked above it, by the same LDS rule ...
    moved = 0
    for n in (17, 25, 32, 33, 48, 49, 64):
        for k in (n, 64, 128, 256, 257, 288, 289, 416, 417, 608, 609, NKV_MAX_COLS):
            if k < n:
                continue
            a, b = rotate_plan(lo, k, n), rotate_plan(hi, k, n)
            assert a == expected_plan(k, n, LD_LAST_32) and b == expected_plan(k, n, LD_FIRST_64), (k, n)
            assert b[0] != "wide"
            moved += a[0] == "wide"
            if a[0] != "wide":
                assert a == b, (k, n)
    assert moved > 20
    # ... and no other path's plan changes across it
    for k, n in [(7, 3), (64, 16), (1000, 11), (417, 20), (609, 20), (257, 64), (300, 64), (83, 70), (128, 128),
                 (200, 128), (300, 150), (576, 256)]:
        a = rotate_plan(lo, k, n)
        assert a[0] != "wide" and a == rotate_plan(hi, k, n) == rotate_plan(SMALL, k, n), (k, n)


# ---- argument errors: nkv_rotate_cols's checks, from the one place that makes them ------------------
def _raw(L, k, ldv, n_out, outs=None):
    o = [ctypes.c_int(-7) for _ in range(4)]
    ptrs = [ctypes.byref(x) for x in o] if outs is None else outs
    rc = _lib.load().nkv_rotate_plan(None if L is None else ctypes.byref(L), k, ldv, n_out, *ptrs)
    return rc, [x.value for x in o]


@pytest.mark.parametrize("k,ldv,n_out,code,word", [
    (0, 4, 1, NKV_EINVAL, "k=0"), (-3, 4, 1, NKV_EINVAL, "k=-3"),
    (NKV_MAX_COLS + 1, NKV_MAX_COLS + 1, 6, NKV_EINVAL, "k=1025"),
    (8, 7, 4, NKV_EINVAL, "ldv=7"),
    (4, 4, 0, NKV_EINVAL, "n_out=0"), (4, 4, -1, NKV_EINVAL, "n_out=-1"), (4, 4, 5, NKV_EINVAL, "n_out=5"),
    (300, 300, NKV_ROT_MAX_OUT + 1, NKV_ESHAPE, "NKV_ROT_MAX_OUT"), (600, 600, 600, NKV_ESHAPE, "NKV_ROT_MAX_OUT"),
])
def test_argument_errors(k, ldv, n_out, code, word):
    """The statuses include/nekkrylov.h documents for nkv_rotate_cols (tests/test_gpu_kernels.py asserts them
    on the launcher; tests/test_gpu_rotate_paths.py that the two agree); the outputs are left alone."""
    rc, out = _raw(SMALL.c_struct(), k, ldv, n_out)
    assert rc == code and out == [-7] * 4
    assert word in _lib.last_error()


def test_null_and_bad_layout_errors():
    L = SMALL.c_struct()
    assert _raw(None, 8, 8, 4)[0] == NKV_EINVAL
    bad = SMALL.c_struct()
    bad.ld += 8                                         # not a multiple of NKV_TILE
    assert _raw(bad, 8, 8, 4)[0] == NKV_ESHAPE
    o = [ctypes.c_int(0) for _ in range(4)]
    for missing in range(4):
        ptrs = [None if i == missing else ctypes.byref(x) for i, x in enumerate(o)]
        assert _raw(L, 8, 8, 4, ptrs)[0] == NKV_EINVAL
        assert "NULL" in _lib.last_error()
    assert _raw(L, 8, 8, 4)[0] == NKV_OK
    assert _raw(L, 8, 11, 4) == (NKV_OK, [_lib.NKV_ROT_PATH_FEW, 4, 256, 2048])   # ldv > k is fine


def test_helper_and_constants():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "nekkrylov.h")).read()
    defs = dict(re.findall(r"#define (NKV_ROT_PATH_[A-Z]+)\s+(\d+)", txt))
    assert {k: int(v) for k, v in defs.items()} == {
        "NKV_ROT_PATH_FEW": _lib.NKV_ROT_PATH_FEW, "NKV_ROT_PATH_WIDE": _lib.NKV_ROT_PATH_WIDE,
        "NKV_ROT_PATH_STREAM": _lib.NKV_ROT_PATH_STREAM, "NKV_ROT_PATH_CHUNKED": _lib.NKV_ROT_PATH_CHUNKED}
    assert sorted(ROTATE_PATHS.values()) == ["chunked", "few", "stream", "wide"]
    assert rotate_plan(SMALL, 128, 25) == rotate_plan(SMALL.c_struct(), 128, 25, ldv=131) == ("wide", 2, 512, 256)
    with pytest.raises(_lib.NkvError) as e:
        rotate_plan(SMALL, 4, 5)
    assert e.value.code == NKV_EINVAL
    assert _lib.load().nkv_abi_version() == 3            # an added entry point does not bump the ABI
