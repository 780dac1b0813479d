// nkv_internal.h — shared by the translation units of libnekkrylov.so (not installed; the public
// C ABI is include/nekkrylov.h).  Tuning knobs, error plumbing, layout helpers and the CDNA4 device
// helpers every kernel family uses (wave64 reductions, 16-byte streaming loads/stores).
//
// Every kernel of the library is HBM-bound fp64 streaming (BLAS-1/2) except the restart rotation
// (f64 MFMA): 16-B (double2) coalesced loads, 256-thread workgroups (4 wave64s), wave reductions by
// cross-lane shuffles and DPP, LDS for the per-workgroup partials, and a deterministic two-stage
// reduction (fixed block->tile map, fixed-order second stage; no floating-point atomics) so results
// do not depend on timing.  Layout, flags and the reference functions each entry point replaces:
// include/nekkrylov.h.  Rooflines and bytes per launch: DESIGN.md §4.
//
// Translation units (one kernel family each, linked into one .so by __graft_entry__.build()):
//   core.hip          error state, device info, workspace, NaN status
//   vector.hip        BLAS-1, weighted dots / multi-dot, second-stage reduction, normalise, MGS column step
//   gram_schmidt.hip  block updates, fused CGS2 pass, DCGS2 multi-dot / coefficients / dual update,
//                     GKL coefficients, MGS in inverse compact WY form
//   rotate.hip        Krylov–Schur restart rotation Q <- Q V (VALU few-column, f64 MFMA stream/chunked)
//   drivers.hip       one-call factorisations (DCGS2, CGS2/MGS2, MGS2-ICWY), GMRES cycle, Givens column
//   operators.hip     synthetic operators and the hashed test vectors
//   sensitivity.hip   seed noise (mth_rand), symmetric seed, wave-maker, gradm1, base-flow sensitivity
//   fixedp.hip        fixed-point forcing: fused SFD step, TDF step on a ring slot (residual from the same pass)
//   postproc.hip      eigenmode kinetic-energy budget: fused production terms + integrals, divergence, dissipation
//   vortex.hip        flow diagnostics: fused vortex criteria (+ filter_s0 in LDS), standalone filter_s0,
//                     energy / enstrophy component sums
//   forcing.hip       body-force hooks: sponge function + masked dot weights, fused force assembly (SFD/TDF
//                     forcing + harmonic resolvent forcing + sponge term) per time step
//   monitors.hip      per-step monitors: surface forces on the member faces of an object (lift / drag / torque),
//                     running mean, mean-square and cross-moment statistics in one pass
//   gs.hip            sharded gather-scatter: pack of the shared points, direct-stiffness average of many
//                     field segments per launch from local points and the values other ranks sent
//   advdiff.hip       spectral-element advection-diffusion of the dotted fields by a frozen base flow: fused
//                     weak-form right-hand side (forward and adjoint), mass matrix, Horner stage / projector halves,
//                     complex Horner stage of the rotating-frame resolvent (re / im halves, forcing inside);
//                     the convection linearised about a base state (production term, forward and adjoint) and
//                     the classical RK4 stage of the viscous Burgers flow
//   pressure.hip      the pressure operators of the incompressible flow on the P_N - P_{N-2} pair: weak divergence
//                     onto the Gauss mesh, its transpose, and the pointwise third of the CG iteration of the
//                     divergence-free projection (deterministic partials, scalars on the device)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nekkrylov.h"

// Tuning knobs (compile-time; tools/tune_kernels.py builds variants and times them on MI355X):
#ifndef NKV_PAIRS
#define NKV_PAIRS 8  // double2 per thread per tile in the dot/update kernels (large problems)
#endif
#ifndef NKV_PAIRS_SMALL
#define NKV_PAIRS_SMALL 4  // ... when the vector has fewer than NKV_SMALL_TILES large tiles (4: +9-13 % on the
                           // multi-dot at N=2e6 over 2, profiles/r01m_tune_small.log)
#endif
#ifndef NKV_SMALL_TILES
#define NKV_SMALL_TILES 2048
#endif
#ifndef NKV_COLU
#define NKV_COLU 4  // basis columns in flight per thread in the multi-dot
#endif
#ifndef NKV_NT
#define NKV_NT 1  // non-temporal loads for the streamed basis columns
#endif
#ifndef NKV_MAXB
#define NKV_MAXB 1024  // workgroups (= reduction partials per column) of the dot/update kernels
#endif
#ifndef NKV_FUSE_NW
#define NKV_FUSE_NW 8  // waves per workgroup of the fused update+dot for j <= 16*NKV_FUSE_NW
#endif
#ifndef NKV_FUSE_G
#define NKV_FUSE_G 1024  // workgroups of the fused update+dot
#endif
#ifndef NKV_FUSE_G_MID
#define NKV_FUSE_G_MID 512  // ... for NKV_FUSE_MID_LO <= j <= NKV_FUSE_MID_HI: +5-8 % at N = 1.25e7,
#endif                      // 5e7 and 1e8 (profiles/r02ao_tune_fmid.log)
#ifndef NKV_FUSE_MID_LO
#define NKV_FUSE_MID_LO 16
#endif
#ifndef NKV_FUSE_MID_HI
#define NKV_FUSE_MID_HI 32
#endif
#ifndef NKV_DC_PAIRS
#define NKV_DC_PAIRS 8  // double2 per thread per tile in the DCGS2 kernels (large problems)
#endif
#ifndef NKV_DC_U
#define NKV_DC_U 2  // basis columns in flight in the DCGS2 dual update
#endif
#ifndef NKV_NT_ST
#define NKV_NT_ST 1  // non-temporal stores of streamed vectors (DCGS2 update, finish, synthetic matvec)
#endif
#ifndef NKV_STREAM_UNR
#define NKV_STREAM_UNR 4  // double2 per thread in flight in the streaming vector kernels
#endif
#ifndef NKV_DC_G
#define NKV_DC_G 768  // workgroups of the DCGS2 dual update: 3 per CU (122 VGPRs allow 4) is 1-6 %
                      // faster than 4 per CU at N=1e8 and at the 8-GPU shard; non-multiples of the
                      // 256 CUs lose 5-10 % (profiles/r01k_tune_update_grid.log)
#endif
#ifndef NKV_UPD_ROUNDS
#define NKV_UPD_ROUNDS 2  // block update (CGS2 passes, DCGS2 close): row-band launches of this many rounds
#endif                    // (+2 % on update+norm at N=1e8, profiles/r02bh_tune_upd_bands.log)
#ifndef NKV_AXD_ROUNDS
#define NKV_AXD_ROUNDS 0  // fused MGS column step (nkv_axpy_dot): row-band launches of this many rounds
#endif
#ifndef NKV_UPD_SMALL_J
#define NKV_UPD_SMALL_J 2   // block update: 4x the workgroups up to this many columns (+5-9 % at j <= 2,
                            // neutral to -4 % from j = 4 on: profiles/r02br_tune_upd_small*.log)
#endif
#ifndef NKV_FUSE_SMALL_J
#define NKV_FUSE_SMALL_J 12  // fused CGS2 middle pass: 4-wave workgroups up to this many columns
#endif                       // (profiles/r02bn_tune_fuse_small*.log); 0 disables
static_assert(NKV_FUSE_SMALL_J >= 0 && NKV_FUSE_SMALL_J <= 16,
              "the 4-wave fused pass instantiates at most 16 columns (NKV_FUSE(4, 4))");
#ifndef NKV_FUSE_ROUNDS
#define NKV_FUSE_ROUNDS 0  // fused CGS2 middle pass: row-band launches of this many rounds (0: one launch)
#endif
#ifndef NKV_DC_ROUNDS
#define NKV_DC_ROUNDS 2  // DCGS2 updates: one launch per this many grid-stride rounds of row tiles (a
                         // "row band"); the launch boundaries keep the grid's loads and stores in one
                         // band: +9-19 % at N=1e8, +0-1 % at the 8-GPU shard (profiles/r02f_tune_*)
#endif
#ifndef NKV_STREAM_ROUNDS
#define NKV_STREAM_ROUNDS 2  // synthetic diagonal matvec: one launch per this many grid-stride rounds
#endif
#ifndef NKV_D2_MAXB
#define NKV_D2_MAXB 256  // workgroups of the two-vector multi-dot: one per CU (+1 % over 1024 at
                          // N=1e8 and at the 8-GPU shard; 384 = 1.5 per CU loses 6-10 %)
#endif
#ifndef NKV_D2_SMALL_B
#define NKV_D2_SMALL_B 512  // ... and for small problems (2-row tiles, no field loop): two per CU; the
                            // kMaxBlocks grid (one tile per block) loses 10-27 % at N=2e6
                            // (profiles/r03aa_tune_d2_small_grid.log)
#endif
#ifndef NKV_DOT_SMALL_B
#define NKV_DOT_SMALL_B 512  // workgroups of the one-vector multi-dot / dot on small problems: as the
                            // two-vector one, +6-12 % at N=2e6, j >= 4 (profiles/r03ac_tune_dot_small_grid.log)
#endif
#ifndef NKV_D2_FIELDLOOP
#define NKV_D2_FIELDLOOP 1  // two-vector multi-dot: one block walks all weighted fields of a tile
#endif
#ifndef NKV_D2_U
#define NKV_D2_U 2  // basis columns in flight in the two-vector multi-dot
#endif
#ifndef NKV_D2_PAIRS
#define NKV_D2_PAIRS NKV_DC_PAIRS  // double2 per thread per tile in the two-vector multi-dot (large problems)
#endif
// The round-1 timing experiments (store skipping, grid-wide soft barriers, tile-interleaved and
// field-major sweeps, XCD tile maps, buffer-store cache policies, register-budget schedules;
// CHANGELOG.md, "What did not help") are not part of this file.  The knobs above change speed only.
#if defined(NKV_DC_EXPERIMENT) || defined(NKV_DC_SYNC) || defined(NKV_QTILE_EXP) || defined(NKV_D2_FIELDMAJOR) || \
    defined(NKV_DC_SCHED) || defined(NKV_D2_SCHED) || defined(NKV_ST_AUX) || defined(NKV_XCD_MAP) ||           \
    defined(NKV_DC_FIELDLOOP) || defined(NKV_FUSE_PF) || defined(NKV_LD_ALIGN)
#error "round-1 experiment switches were removed from the product kernel"
#endif

// ---- cross-TU host helpers (hidden: not part of the exported ABI) -------------------------------
#pragma GCC visibility push(hidden)
namespace nkvi {
// Record an error message for nkv_last_error() and return `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Compute units of the current device (cached per device id; 256 on MI355X).
int device_cus();
int check_layout(const nkv_layout* L);
int check_ptr(const void* p, const char* what);
// Weighted multi-dot h = Q^T W f over j columns (+ the second stage), the j = 1 case is nkv_dot.
int launch_block_dot(const nkv_layout* L, const double* w, const double* Q, int64_t ld, int j, const double* f,
                     double* out, void* ws, unsigned flags, hipStream_t st);
// Second stage of every reduction: out[c] = sum_b partials[c][b] in a fixed order, c < ncols
// (+ the replicated time term ta[c] tb / ta[c - jc] tb2; NaN -> flag).
int launch_reduce_cols(int ncols, const double* partials, int B, double* out, const double* ta, int64_t lda,
                       const double* tb, const double* tb2, int jc, int* nan_flag, hipStream_t st);
}  // namespace nkvi
#pragma GCC visibility pop
using namespace nkvi;

#define NKV_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(NKV_EHIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,  \
                        __LINE__);                                                           \
    } while (0)

#define NKV_LAUNCHED()                                                                       \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess)                                                                \
            return fail(NKV_EHIP, "kernel launch: %s (%s:%d)", hipGetErrorString(e_),        \
                        __FILE__, __LINE__);                                                 \
    } while (0)

#define CHECK(x)                   \
    do {                           \
        int rc_ = (x);             \
        if (rc_ != NKV_OK) return rc_; \
    } while (0)

namespace {

constexpr int kThreads = 256;                       // 4 waves of 64
constexpr int kStreamUnr = NKV_STREAM_UNR;
static_assert(NKV_TILE % (2 * kThreads * NKV_STREAM_UNR) == 0, "stream chunk must divide the padding");
static_assert(NKV_TILE % (kThreads * NKV_PAIRS * 2) == 0, "kernel tile must divide the padding");
static_assert(NKV_TILE % (kThreads * NKV_PAIRS_SMALL * 2) == 0, "kernel tile must divide the padding");
constexpr int kMaxBlocks = NKV_MAXB;                 // reduction partial slots per column
constexpr int kColUnroll = NKV_COLU;                 // columns in flight per thread (block dot)
constexpr size_t kCtrlBytes = 256;                   // control words at the head of the workspace
constexpr int kFuseRows = 128;                       // rows per tile of the fused CGS2 middle pass (k_update_dot)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Rows that every BLAS-1 op streams (weighted fields + pressure, padded); the time slot sits at
// this offset.
inline int64_t rows_of(const nkv_layout* L) { return (int64_t)L->n_wf * L->sv + L->sp; }

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

#ifndef NKV_D2_RED
#define NKV_D2_RED 1  // transposed wave reduction in the multi-dots (DPP within rows): +4-10 % on
                      // the two-vector dot at N=2e6, +0.3 % at N=1e8 (profiles/r01m_tune_d2red.log)
#endif

// One DPP move of a double (two 32-bit halves), every lane reading its source lane.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(__double_as_longlong(v) & 0xffffffffll), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(__double_as_longlong(v) >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Sums of FOUR per-lane values over the 64 lanes in 7 exchanges instead of 24: the xor-32 and
// xor-16 steps each hand half of the values to the partner (so every lane keeps one value from
// there on), the in-row steps run on DPP (quad xor 1, quad xor 2, half-row mirror, row mirror).
// Value v lands in lane 16 v (v = 0..3).  Deterministic (a fixed exchange pattern).
__device__ __forceinline__ double wave_sum4(double s0, double s1, double s2, double s3, int lane) {
    const bool up = (lane & 32) != 0;
    const double k0 = (up ? s2 : s0) + __shfl_xor(up ? s0 : s2, 32, 64);
    const double k1 = (up ? s3 : s1) + __shfl_xor(up ? s1 : s3, 32, 64);
    const bool b4 = (lane & 16) != 0;
    double v = (b4 ? k1 : k0) + __shfl_xor(b4 ? k0 : k1, 16, 64);
    v += dpp_d<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v);   // row_half_mirror
    v += dpp_d<0x140>(v);   // row_mirror
    return v;
}

// Block-wide sum of one double (256 threads); result valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* lds4) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) lds4[wave] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
    return r;
}

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
// uniform base + 32-bit byte offset: lets the compiler use the SGPR-base/VGPR-offset load form
// instead of a 64-bit VGPR address per column (fewer VGPRs in the register-resident kernels)
__device__ __forceinline__ const double* at_b(const double* base, uint32_t byte_off) {
    return reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + byte_off);
}

typedef double v2d __attribute__((ext_vector_type(2)));
// Loads of streamed basis columns: each byte is read once per pass and, at the sizes that matter,
// the basis is far larger than L2 + Infinity Cache, so the loads are non-temporal (NKV_NT).
__device__ __forceinline__ double2 ldq(const double* p) {
#if NKV_NT
    const v2d v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p));
    return make_double2(v.x, v.y);
#else
    return ld2(p);
#endif
}
__device__ __forceinline__ void st2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }
// Stores of whole streamed vectors (800 MB at N=1e8, never re-read from cache): non-temporal (NKV_NT_ST)
__device__ __forceinline__ void st2s(double* p, double2 v) {
#if NKV_NT_ST
    __builtin_nontemporal_store(v2d{v.x, v.y}, reinterpret_cast<v2d*>(p));
#else
    st2(p, v);
#endif
}
// Store of one double2 at element offset `off` of a streamed vector `base`.
__device__ __forceinline__ void st2p(double* base, int64_t off, double2 v) { st2s(base + off, v); }

#ifndef NKV_STREAM_G
#define NKV_STREAM_G 4096  // workgroup cap of the streaming kernels (op_diag, finish, BLAS-1)
#endif
inline int grid_for(int64_t work_items, int cap = NKV_STREAM_G) {
    int64_t g = (work_items + kThreads - 1) / kThreads;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

struct Ctrl {
    int nan_flag;
};

inline int* nan_flag_of(void* ws) { return &reinterpret_cast<Ctrl*>(ws)->nan_flag; }
inline double* partials_of(void* ws) {
    return reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + kCtrlBytes);
}

// Rows per thread: NKV_PAIRS*2 when the vector has enough large tiles to fill the chip, else fewer.
inline bool use_large_tiles(const nkv_layout* L) {
    return rows_of(L) / (kThreads * NKV_PAIRS * 2) >= NKV_SMALL_TILES;
}

// ------------------------------------------------------------------------------------------
// The element tile of k_gradm1 (sensitivity.hip), shared by the tiled element kernels of postproc.hip
// and vortex.hip: whole elements per workgroup, whole waves, one point per thread.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
constexpr int tile_pts() { return LDIM == 3 ? NX * NX * NX : NX * NX; }
template <int LDIM, int NX>
constexpr int tile_threads() {
    return tile_pts<LDIM, NX>() >= 256 ? (tile_pts<LDIM, NX>() + 63) / 64 * 64 : 256;
}
inline int tile_epb(int pts) { return pts >= 256 ? 1 : 256 / pts; }
constexpr int kMaxWaves = 16;   // 1024 threads (lx1 = 10 in 3-D: 1000 points)

// This thread's point of the tile: its element, its indices, its three lines, its rows and its columns of D (LDS).
// The lines and rows take the point's indices from its offset r inside its element, as k_gradm1 does; i, j, k and
// the columns take them from tid, where the element drops out because NX and NX^2 divide the points of an
// element.  The values are the same.  Sharing one chain costs the tiled kernels of advdiff.hip registers at the
// 4-wave budget (a column pointer off tid is rematerialised, one off r is kept live): CHANGELOG, "Shared element-tile
// building blocks".
template <int LDIM, int NX>
struct TilePoint {
    int i, j, k;                    // the point inside its element
    int ri, si, ti;                 // lines along r, s, t through the point
    const double *Di, *Dj, *Dk;     // rows of D: D(i, m) at Di[m]
    const double *Ci, *Cj, *Ck;     // columns of D: D(m, i) at Ci[m*NX]
    __device__ __forceinline__ TilePoint(const double* D, int tid, int nt) {
        constexpr int pts = tile_pts<LDIM, NX>();
        const int le = tid / pts, r = tid - le * pts;
        const int ir = r % NX, jr = (r / NX) % NX, kr = LDIM == 3 ? r / (NX * NX) : 0;
        const int base = (tid < nt ? le : 0) * pts;   // lanes past the last whole element read element 0
        ri = base + jr * NX + kr * NX * NX;
        si = base + ir + kr * NX * NX;
        ti = base + ir + jr * NX;
        Di = D + ir * NX;
        Dj = D + jr * NX;
        Dk = D + kr * NX;
        i = tid % NX;
        j = (tid / NX) % NX;
        k = LDIM == 3 ? (tid / (NX * NX)) % NX : 0;
        Ci = D + i;
        Cj = D + j;
        Ck = D + k;
    }
    // The product of the point's GLL weights w_i w_j [w_k].
    __device__ __forceinline__ double weight(const double* w) const {
#pragma clang fp contract(off)
        const double wij = w[i] * w[j];
        return LDIM == 3 ? wij * w[k] : wij;
    }
};

// glmapm1 / xyzrst's geometric factors of one point from the staged coordinates: the arithmetic of
// k_gradm1, operation for operation (mxm line sums with m ascending, addcol4 / subcol4 Jacobian,
// ascol5 cofactors).  g[direction][reference coordinate r, s, t].
template <int LDIM, int NX>
__device__ __forceinline__ void geometric_factors_jac(const TilePoint<LDIM, NX>& q, const double* X, const double* Y,
                                                      const double* Z, double (&g)[3][3], double& jac_out) {
#pragma clang fp contract(off)
    constexpr int sj = NX, sk = NX * NX;
    const double *Di = q.Di, *Dj = q.Dj, *Dk = q.Dk;
    const int ri = q.ri, si = q.si, ti = q.ti;
    double xr = Di[0] * X[ri], yr = Di[0] * Y[ri];
    double xs = X[si] * Dj[0], ys = Y[si] * Dj[0];
#pragma unroll 2
    for (int m = 1; m < NX; ++m) {
        xr = xr + Di[m] * X[ri + m];
        yr = yr + Di[m] * Y[ri + m];
        xs = xs + X[si + m * sj] * Dj[m];
        ys = ys + Y[si + m * sj] * Dj[m];
    }
    if constexpr (LDIM == 2) {
        double jac = 0.0;
        jac = jac + xr * ys;
        jac = jac - xs * yr;
        g[0][0] = ys;
        g[1][0] = -xs;
        g[0][1] = -yr;
        g[1][1] = xr;
        jac_out = jac;
    } else {
        double zr = Di[0] * Z[ri], zs = Z[si] * Dj[0];
        double xt = X[ti] * Dk[0], yt = Y[ti] * Dk[0], zt = Z[ti] * Dk[0];
#pragma unroll 2
        for (int m = 1; m < NX; ++m) {
            zr = zr + Di[m] * Z[ri + m];
            zs = zs + Z[si + m * sj] * Dj[m];
            xt = xt + X[ti + m * sk] * Dk[m];
            yt = yt + Y[ti + m * sk] * Dk[m];
            zt = zt + Z[ti + m * sk] * Dk[m];
        }
        double jac = 0.0;
        jac = jac + xr * ys * zt;
        jac = jac + xt * yr * zs;
        jac = jac + xs * yt * zr;
        jac = jac - xr * yt * zs;
        jac = jac - xs * yr * zt;
        jac = jac - xt * ys * zr;
        g[0][0] = ys * zt - yt * zs;   // rx
        g[1][0] = xt * zs - xs * zt;   // ry
        g[2][0] = xs * yt - xt * ys;   // rz
        g[0][1] = yt * zr - yr * zt;   // sx
        g[1][1] = xr * zt - xt * zr;   // sy
        g[2][1] = xt * yr - xr * yt;   // sz
        g[0][2] = yr * zs - ys * zr;   // tx
        g[1][2] = xs * zr - xr * zs;   // ty
        g[2][2] = xr * ys - xs * yr;   // tz
        jac_out = jac;
    }
}

// ... and the inverse Jacobian every derivative is scaled by (jacmi = 1 / jac, as k_gradm1 forms it).
template <int LDIM, int NX>
__device__ __forceinline__ void geometric_factors(const TilePoint<LDIM, NX>& q, const double* X, const double* Y,
                                                  const double* Z, double (&g)[3][3], double& jacmi) {
#pragma clang fp contract(off)
    double jac;
    geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
    jacmi = 1.0 / jac;
}

// ur, us, [ut] of one staged field at this point (k_gradm1's line sums).
template <int LDIM, int NX>
__device__ __forceinline__ void line_sums(const TilePoint<LDIM, NX>& q, const double* U, double& ur, double& us,
                                          double& ut) {
#pragma clang fp contract(off)
    constexpr int sj = NX, sk = NX * NX;
    ur = q.Di[0] * U[q.ri];
    us = U[q.si] * q.Dj[0];
    ut = 0.0;
#pragma unroll 2
    for (int m = 1; m < NX; ++m) {
        ur = ur + q.Di[m] * U[q.ri + m];
        us = us + U[q.si + m * sj] * q.Dj[m];
    }
    if constexpr (LDIM == 3) {
        ut = U[q.ti] * q.Dk[0];
#pragma unroll 2
        for (int m = 1; m < NX; ++m) ut = ut + U[q.ti + m * sk] * q.Dk[m];
    }
}

// The transpose of line_sums: sum_a D_a^T of the three flux tiles at this point,
//   sum_m D(m, i) X(m, j, k) + sum_m D(m, j) Y(i, m, k) [+ sum_m D(m, k) Z(i, j, m)],  m ascending.
template <int LDIM, int NX>
__device__ __forceinline__ double transposed_line_sums(const TilePoint<LDIM, NX>& q, const double* X, const double* Y,
                                                       const double* Z) {
#pragma clang fp contract(off)
    constexpr int sj = NX, sk = NX * NX;
    double tr = q.Ci[0] * X[q.ri], ts = Y[q.si] * q.Cj[0];
#pragma unroll 2
    for (int m = 1; m < NX; ++m) {
        tr = tr + q.Ci[m * NX] * X[q.ri + m];
        ts = ts + Y[q.si + m * sj] * q.Cj[m * NX];
    }
    double acc = tr + ts;
    if constexpr (LDIM == 3) {
        double tt = Z[q.ti] * q.Ck[0];
#pragma unroll 2
        for (int m = 1; m < NX; ++m) tt = tt + Z[q.ti + m * sk] * q.Ck[m * NX];
        acc = acc + tt;
    }
    return acc;
}

// The derivative along direction d exactly as k_gradm1 stores it: jacmi * acc.
template <int LDIM>
__device__ __forceinline__ double physical_derivative(const double (&g)[3][3], double jacmi, int d, double ur,
                                                      double us, double ut) {
#pragma clang fp contract(off)
    const double acc = LDIM == 3 ? ur * g[d][0] + us * g[d][1] + ut * g[d][2] : ur * g[d][0] + us * g[d][1];
    return jacmi * acc;
}

// The argument checks the tiled element entries share with nkv_gradm1.
inline int check_mesh_args(const char* who, const nkv_layout* L, int lx1, int ldim, const double* zm) {
    if (ldim != 2 && ldim != 3) return fail(NKV_EINVAL, "%s: ldim=%d must be 2 or 3", who, ldim);
    if (lx1 < 2 || lx1 > 10) return fail(NKV_EINVAL, "%s: lx1=%d outside 2..10", who, lx1);
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    if (L->n_v % pts != 0)
        return fail(NKV_EINVAL, "%s: %d points per element (lx1=%d) do not divide n_v=%lld", who, pts, lx1,
                    (long long)L->n_v);
    if ((ldim == 3) != (zm != nullptr)) return fail(NKV_EINVAL, "%s: zm must be given exactly in 3-D", who);
    return NKV_OK;
}

inline int need(const void* p, const char* who, const char* what) {
    if (!p) return fail(NKV_EINVAL, "%s: %s is NULL", who, what);
    return NKV_OK;
}

// One switch case per supported lx1 (template parameter NX) of the tiled element kernels.
#define NKV_PP_CASES(CALL) \
    CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8) CALL(9) CALL(10)

}  // namespace
