// core.hip — error state, device info, workspace sizing and the NaN status of the C ABI.
#include "nkv_internal.h"

namespace nkvi {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// Compute units of the current device (cached per device id; 256 on MI355X).
int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
                       ? n : 256;
    }
    return cus[dev];
}

int check_layout(const nkv_layout* L) {
    if (!L) return fail(NKV_EINVAL, "layout is NULL");
    if (L->n_wf < 1 || L->n_v < 0 || L->n_p < 0)
        return fail(NKV_EINVAL, "bad layout: n_wf=%d n_v=%lld n_p=%lld", L->n_wf,
                    (long long)L->n_v, (long long)L->n_p);
    if (L->sv < L->n_v || L->sp < L->n_p || L->sv % NKV_TILE || L->sp % NKV_TILE || L->ld % NKV_TILE)
        return fail(NKV_ESHAPE, "layout not padded to NKV_TILE: sv=%lld sp=%lld ld=%lld",
                    (long long)L->sv, (long long)L->sp, (long long)L->ld);
    if (L->ld < rows_of(L) + 1)
        return fail(NKV_ESHAPE, "ld=%lld too small for %lld rows + time", (long long)L->ld,
                    (long long)rows_of(L));
    return NKV_OK;
}

int check_ptr(const void* p, const char* what) {
    if (!p) return fail(NKV_EINVAL, "%s is NULL", what);
    if (reinterpret_cast<uintptr_t>(p) % 16) return fail(NKV_ESHAPE, "%s not 16-byte aligned", what);
    return NKV_OK;
}

}  // namespace nkvi

extern "C" {

int nkv_abi_version(void) { return NKV_ABI_VERSION; }

int nkv_layout_init(nkv_layout* L, int ldim, int lx1, int lx2, int64_t nelv, int64_t nelt, int n_scalars,
                    int ifpo, int rank0) {
    if (!L) return fail(NKV_EINVAL, "layout is NULL");
    if ((ldim != 2 && ldim != 3) || lx1 < 2 || (ifpo && lx2 < 1) || nelv < 0 || n_scalars < 0)
        return fail(NKV_EINVAL, "bad layout parameters: ldim=%d lx1=%d lx2=%d nelv=%lld n_scalars=%d", ldim, lx1,
                    lx2, (long long)nelv, n_scalars);
    // k_dot / real_dot weight a scalar over nt = nx1*ny1*nz1*nelt points with bm1s(lx1,ly1,lz1,lelv)
    // (core/krylov_subspace.f90:36-44, nek_vectors.f90:88-99, core/NEKSTAB:86): with nelt != nelv
    // (conjugate heat transfer) the reference reads past its weights, so such a layout is refused
    if (n_scalars > 0 && nelt != nelv)
        return fail(NKV_ESHAPE, "nelt=%lld != nelv=%lld with %d dotted scalar(s): conjugate heat transfer "
                    "layouts are not supported (the reference weights t over nelt elements with the nelv-element "
                    "bm1s, krylov_subspace.f90:36-44, NEKSTAB:86)", (long long)nelt, (long long)nelv, n_scalars);
    int64_t pv = lx1, pp = ifpo ? lx2 : 0;
    for (int d = 1; d < ldim; ++d) {
        pv *= lx1;
        pp *= ifpo ? lx2 : 0;
    }
    auto up = [](int64_t n) { return (n + NKV_TILE - 1) / NKV_TILE * NKV_TILE; };
    L->n_v = pv * nelv;
    L->n_p = pp * nelv;
    L->sv = up(L->n_v);
    L->sp = up(L->n_p);
    L->n_wf = ldim + n_scalars;
    L->ld = up((int64_t)L->n_wf * L->sv + L->sp + 1);
    L->rank0 = rank0 ? 1 : 0;
    return NKV_OK;
}

const char* nkv_last_error(void) { return g_err; }

int nkv_device_info(int* device, int* cu_count, int64_t* hbm_bytes, char* name, int name_len) {
    int dev = 0;
    NKV_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    NKV_HIP(hipGetDeviceProperties(&p, dev));
    if (device) *device = dev;
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    if (name && name_len > 0) {
        snprintf(name, name_len, "%s", p.gcnArchName);
    }
    return NKV_OK;
}

size_t nkv_workspace_bytes(const nkv_layout* L, int max_cols) {
    (void)L;
    if (max_cols < 1) max_cols = 1;
    return kCtrlBytes + (size_t)kMaxBlocks * (size_t)(2 * max_cols + 2) * sizeof(double);  // 2 RHS (DCGS2)
}

// The launch shapes of the streaming entry points, host only: every size threshold and band formula of
// vector.hip's and gram_schmidt.hip's launchers and of nkv_op_diag lives here; the launchers map the plan to
// hipLaunchKernelGGL and decide nothing themselves.  tests/test_stream_plan.py restates the rules.
// One rule is the kernel's own and only restated here: k_dcgs2_update<P, true> runs its per-tile loop when
// tiles_per_field < gridDim.x and m >= 8, its per-unit loop otherwise (gram_schmidt.hip).
// NKV_FUSE_ROUNDS = NKV_AXD_ROUNDS = 0 in the product build: the fused pass and nkv_axpy_dot launch once.
namespace {

// One launch per `rounds` grid-stride rounds of the grid_x-workgroup grid (a row band); every item in one launch
// when banding is off or the loop is shorter than two bands.  The first launch always has the whole grid, so
// every partial slot is written before a later band adds to it; the last launch's grid shrinks to its items
// where `shrink` (op_diag keeps its grid).  At least one launch: the time slot of an empty shard.
void set_bands(nkv_plan* p, int rounds, bool shrink) {
    const int64_t n = p->tiles, g = p->grid_x, b = (int64_t)rounds * g;
    p->band_tiles = (rounds <= 0 || n < 2 * b) ? (n > 0 ? n : 1) : b;
    p->launches = n > 0 ? (n + p->band_tiles - 1) / p->band_tiles : 1;
    const int64_t left = n - (p->launches - 1) * p->band_tiles;
    p->last_grid_x = (p->launches > 1 && shrink && left < g) ? left : g;
}

// The update kernels' 1-D grid over all row tiles of the vector: min(tiles, cap), at least one workgroup.
void set_tile_grid(nkv_plan* p, const nkv_layout* L, int pairs, int64_t cap) {
    p->pairs = pairs;
    p->wg_threads = kThreads;
    p->rows_per_tile = (int64_t)kThreads * pairs * 2;
    p->tiles = rows_of(L) / p->rows_per_tile;
    p->grid_x = p->tiles < cap ? p->tiles : cap;
    if (p->grid_x < 1) p->grid_x = 1;
    p->grid_y = 1;
    p->work_loop = NKV_STREAM_LOOP_TILES;
    p->units = p->tiles;
    p->fields_per_block = 1;
}

}  // namespace

int nkv_stream_plan(const nkv_layout* L, int op, int j, unsigned flags, nkv_plan* plan) {
    CHECK(check_layout(L));
    if (!plan) return fail(NKV_EINVAL, "stream plan: plan is NULL");
    nkv_plan p;
    memset(&p, 0, sizeof(p));
    p.kernel = op;
    const bool large = use_large_tiles(L);   // NKV_PAIRS double2 per thread from NKV_SMALL_TILES large tiles on
    const int64_t rows = rows_of(L);
    switch (op) {
        case NKV_STREAM_BLOCK_DOT:
        case NKV_STREAM_BLOCK_DOT2: {
            if (j < 1 || j > NKV_MAX_COLS) return fail(NKV_EINVAL, "j=%d outside 1..%d", j, NKV_MAX_COLS);
            const bool two = op == NKV_STREAM_BLOCK_DOT2;
            p.pairs = large ? (two ? NKV_D2_PAIRS : NKV_PAIRS) : NKV_PAIRS_SMALL;
            p.wg_threads = kThreads;
            p.rows_per_tile = (int64_t)kThreads * p.pairs * 2;
            p.tiles = L->sv / p.rows_per_tile;
            // two-vector dot, large problems: one block walks every field of its tiles (weights read once per
            // tile); one workgroup per CU (8 rows/thread keep enough loads in flight), two per CU when small.
            // one-vector dot: grid.y = the weighted field; fewer workgroups on small problems
            p.fields_per_block = (two && large && NKV_D2_FIELDLOOP) ? L->n_wf : 1;
            p.grid_y = L->n_wf / p.fields_per_block;
            int64_t bmax = kMaxBlocks;
            if (two) bmax = large ? NKV_D2_MAXB : NKV_D2_SMALL_B;
            else if (!large && NKV_PAIRS_SMALL != NKV_PAIRS) bmax = NKV_DOT_SMALL_B;
            if (bmax > kMaxBlocks) bmax = kMaxBlocks;
            p.grid_x = bmax / p.grid_y;
            if (p.grid_x > p.tiles) p.grid_x = p.tiles;
            if (p.grid_x < 1) p.grid_x = 1;
            p.work_loop = NKV_STREAM_LOOP_TILES;
            p.units = p.tiles;
            p.band_tiles = p.tiles > 0 ? p.tiles : 1;
            p.launches = p.tiles > 0 ? 1 : 0;   // an empty shard: only the second stage (which sums nothing)
            p.last_grid_x = p.grid_x;
            p.partial_slots = p.tiles > 0 ? p.grid_x * p.grid_y : 0;
            p.partial_cols = two ? 2 * j : j;
            break;
        }
        case NKV_STREAM_BLOCK_UPDATE: {
            if (j < 0) return fail(NKV_EINVAL, "j=%d < 0", j);
            // few columns: a 4x larger grid (the norm partials still fit: the workspace holds at least
            // 4 * kMaxBlocks slots, nkv_workspace_bytes with max_cols >= 1)
            set_tile_grid(&p, L, large ? NKV_PAIRS : NKV_PAIRS_SMALL, j <= NKV_UPD_SMALL_J ? 4 * kMaxBlocks : kMaxBlocks);
            set_bands(&p, NKV_UPD_ROUNDS, true);
            if (flags & NKV_NORM2) {
                p.partial_slots = p.grid_x;
                p.partial_cols = 1;
            }
            break;
        }
        case NKV_STREAM_UPDATE_DOT: {
            if (j < 1 || j > NKV_MAX_COLS) return fail(NKV_EINVAL, "j=%d outside 1..%d", j, NKV_MAX_COLS);
            if (j > 256 || rows >= (int64_t)1 << 29) {   // tile does not fit registers / 32-bit offsets
                p.kernel = NKV_STREAM_SPLIT;
                break;
            }
            // 4 waves up to NKV_FUSE_SMALL_J columns, NKV_FUSE_NW up to 16 columns per wave, then 16 waves;
            // mid-size column counts run on a smaller grid
            constexpr int NW = NKV_FUSE_NW;
            p.nw = j <= NKV_FUSE_SMALL_J ? 4 : (j <= NW * 16 ? NW : 16);
            p.cpw = (j + p.nw - 1) / p.nw;
            p.pairs = 1;
            p.wg_threads = p.nw * 64;
            p.rows_per_tile = kFuseRows;
            p.tiles = rows / kFuseRows;
            const int64_t gcap = (j >= NKV_FUSE_MID_LO && j <= NKV_FUSE_MID_HI) ? NKV_FUSE_G_MID : NKV_FUSE_G;
            p.grid_x = p.tiles < gcap ? p.tiles : gcap;
            if (p.grid_x < 1) p.grid_x = 1;
            p.grid_y = 1;
            p.work_loop = NKV_STREAM_LOOP_TILES;
            p.units = p.tiles;
            p.fields_per_block = 1;
            set_bands(&p, NKV_FUSE_ROUNDS, true);
            p.partial_slots = p.grid_x;
            p.partial_cols = j;
            break;
        }
        case NKV_STREAM_DCGS2_UPDATE: {
            if (j < 0) return fail(NKV_EINVAL, "m=%d < 0", j);
            set_tile_grid(&p, L, large ? NKV_DC_PAIRS : NKV_PAIRS_SMALL, NKV_DC_G < kMaxBlocks ? NKV_DC_G : kMaxBlocks);
            if (!(flags & NKV_NORM2)) {
                // one launch per row band: every launch boundary is a grid-wide point where all loads and
                // stores of the band have retired (no in-kernel barrier)
                set_bands(&p, NKV_DC_ROUNDS, true);
                break;
            }
            // with the fused norm every block leaves one partial: a single launch over all tiles
            set_bands(&p, 0, true);
            const int64_t tpf = L->sv / p.rows_per_tile;
            if (!(tpf < p.grid_x && j >= 8)) {   // the kernel's own test (see above)
                p.work_loop = NKV_STREAM_LOOP_UNITS;
                p.units = tpf + (p.tiles - tpf * L->n_wf);
            }
            p.partial_slots = p.grid_x;
            p.partial_cols = 1;
            break;
        }
        case NKV_STREAM_AXPY_DOT: {
            // 4 double2 per thread at every size: +5 % over the 8 of the wide kernels at N=1e8 for this
            // four-stream shape (profiles/r02bl_tune_fewcol.log)
            set_tile_grid(&p, L, NKV_PAIRS_SMALL, kMaxBlocks);
            set_bands(&p, NKV_AXD_ROUNDS, true);
            p.partial_slots = p.tiles > 0 ? p.grid_x : 0;
            p.partial_cols = 1;
            break;
        }
        case NKV_STREAM_BLAS1:
        case NKV_STREAM_FINISH:
        case NKV_STREAM_OP_DIAG: {
            // whole chunks of kStreamUnr double2 per thread (rows is a multiple of NKV_TILE); one thread per row
            // pair up to NKV_STREAM_G workgroups (BLAS-1 counts the time slot's pair too)
            p.pairs = kStreamUnr;
            p.wg_threads = kThreads;
            p.rows_per_tile = (int64_t)2 * kThreads * kStreamUnr;
            p.tiles = rows / p.rows_per_tile;
            p.grid_x = grid_for(op == NKV_STREAM_BLAS1 ? rows / 2 + 1 : rows / 2);
            p.grid_y = 1;
            p.work_loop = NKV_STREAM_LOOP_TILES;
            p.units = p.tiles;
            p.fields_per_block = 1;
            set_bands(&p, op == NKV_STREAM_OP_DIAG ? NKV_STREAM_ROUNDS : 0, false);
            break;
        }
        default:
            return fail(NKV_EINVAL, "stream plan: unknown op %d", op);
    }
    *plan = p;
    return NKV_OK;
}

int nkv_check_status(void* ws, void* stream) {
    CHECK(check_ptr(ws, "ws"));
    int flag = 0;
    NKV_HIP(hipMemcpyAsync(&flag, nan_flag_of(ws), sizeof(int), hipMemcpyDeviceToHost, S(stream)));
    NKV_HIP(hipStreamSynchronize(S(stream)));
    if (flag) {
        NKV_HIP(hipMemsetAsync(nan_flag_of(ws), 0, sizeof(int), S(stream)));
        return fail(NKV_ENAN, "NaN detected in dot product");  // nek_vectors.f90:108-111
    }
    return NKV_OK;
}

}  // extern "C"
