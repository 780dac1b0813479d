// postproc.hip — the eigenmode kinetic-energy budget on the device (stability_energy_budget,
// postproc.f90:649-872): the nine production terms with their integrals in one tiled pass
// (compute_production, :801-836), the element-local divergence that closes a Laplacian
// (compute_laplacian, :853-872) and the fused dissipation term with its integral
// (compute_dissipation, :761-799).
//
// The reference differentiates the base flow three times, forms nine pointwise products and sweeps
// each with glsc2 (:716-730); its six Laplacians are 24 gradm1 calls with three dsavg each, of which
// two thirds of the derivatives are thrown away (:864-867).  Here production is one pass (13 doubles
// read, 9 written per point in 3-D) and a Laplacian is one gradient, one divergence and two averaging
// passes.
#include "nkv_internal.h"

namespace {

// The tile (tile_pts, tile_threads, tile_epb, TilePoint) and the element arithmetic (geometric_factors,
// line_sums, physical_derivative) are nkv_internal.h's: vortex.hip builds on the same copy.

// ------------------------------------------------------------------------------------------
// compute_production (postproc.f90:801-836) for all base components at once, with the glsc2 of
// every term (:728-730) out of the same pass.  Per point, for base component c and direction d:
//   dc/dx_d = gradm1 of base_c (no dsavg, :814/:821/:828), in LDS
//   P[c][d] = -0.5 (re_c re_d + im_d im_c) dc/dx_d     (diagonal: re_c**2 + im_c**2)
//   acc[c][d] += bm1 P[c][d]
// The coordinates and the LDIM base components of a group of whole elements are staged once; the
// factors are formed once per element group.  partials[q * gridDim.x + block] for term q = c LDIM + d.
// ------------------------------------------------------------------------------------------
// Occupancy: the nine accumulators on top of k_gradm1's registers come to 138-146 VGPRs in 3-D, three
// waves per SIMD, i.e. ONE 512-thread workgroup per CU at lx1 = 8.  Asking for four waves per SIMD (128
// VGPRs, 24 bytes of scratch) fits two: 0.72 -> 0.47 ms at lx1 = 8, E = 22,088
// (profiles/energy_budget_occupancy.log).  Workgroups above 512 threads (lx1 = 9, 10) keep the default.
template <int LDIM, int NX>
constexpr int production_min_waves() { return tile_threads<LDIM, NX>() <= 512 ? 4 : 0; }

template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>()), (production_min_waves<LDIM, NX>())) void k_pke_production(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ xm, const double* __restrict__ ym,
    const double* __restrict__ zm, const double* __restrict__ ubase, int64_t b_stride, const double* __restrict__ dRe,
    const double* __restrict__ dIm, int64_t m_stride, const double* __restrict__ bm1, double* __restrict__ prod,
    int64_t p_stride, double* __restrict__ partials) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    __shared__ double red[kMaxWaves][LDIM * LDIM];
    constexpr int pts = tile_pts<LDIM, NX>();
    const int nt = epb * pts;
    double* D = lds;                         // D(i, m) at D[i*NX + m]
    double* X = D + NX * NX;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    double* U = LDIM == 3 ? Z + nt : Z;      // LDIM base components, nt each
    const int tid = threadIdx.x;
    for (int t = tid; t < NX * NX; t += blockDim.x) D[t] = Dg[t];
    const TilePoint<LDIM, NX> q(D, tid, nt);
    const int le = tid / pts;
    double acc[LDIM * LDIM];
#pragma unroll
    for (int t = 0; t < LDIM * LDIM; ++t) acc[t] = 0.0;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = tid < nt && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and D is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
#pragma unroll
            for (int c = 0; c < LDIM; ++c) U[c * nt + tid] = ubase[c * b_stride + p];
        }
        __syncthreads();
        double g[3][3], jacmi;   // dead lanes compute garbage they never use
        geometric_factors<LDIM, NX>(q, X, Y, Z, g, jacmi);
        if (live) {
            double re[LDIM], im[LDIM];
#pragma unroll
            for (int c = 0; c < LDIM; ++c) {
                re[c] = dRe[c * m_stride + p];
                im[c] = dIm[c * m_stride + p];
            }
            const double w = bm1[p];
#pragma unroll
            for (int c = 0; c < LDIM; ++c) {
                double ur, us, ut;
                line_sums<LDIM, NX>(q, U + c * nt, ur, us, ut);
#pragma unroll
                for (int d = 0; d < LDIM; ++d) {
                    const double dcd = physical_derivative<LDIM>(g, jacmi, d, ur, us, ut);
                    const double m2 = c == d ? re[c] * re[c] + im[c] * im[c] : re[c] * re[d] + im[d] * im[c];
                    const double P = -0.5 * m2 * dcd;
                    if (prod) prod[(int64_t)(c * LDIM + d) * p_stride + p] = P;
                    acc[c * LDIM + d] = acc[c * LDIM + d] + w * P;
                }
            }
        }
    }
    // fixed-order block reduction: lanes of a wave, then the waves in ascending order
    const int wave = tid >> 6, lane = tid & 63, nw = (int)blockDim.x >> 6;
#pragma unroll
    for (int t = 0; t < LDIM * LDIM; ++t) {
        const double v = wave_sum(acc[t]);
        if (lane == 0) red[wave][t] = v;
    }
    __syncthreads();
    if (tid < LDIM * LDIM) {
        double s = 0.0;
        for (int wv = 0; wv < nw; ++wv) s = s + red[wv][tid];
        partials[(int64_t)tid * gridDim.x + blockIdx.x] = s;
    }
}

// ------------------------------------------------------------------------------------------
// Divergence of nvec vector fields (component d of vector v at g + (v LDIM + d) g_stride):
//   div_v = (d g_vx/dx + d g_vy/dy) [+ d g_vz/dz]
// each partial derivative exactly what k_gradm1 writes for that field and direction.  With the
// averaged first derivatives of a mode component as the vector this is the sum d2x + d2y + d2z of
// compute_laplacian (postproc.f90:865-869) before its dsavg.  The factors are formed once per element
// group for all nvec vectors.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_divm1(
    int64_t nel, int epb, int nvec, const double* __restrict__ Dg, const double* __restrict__ xm,
    const double* __restrict__ ym, const double* __restrict__ zm, const double* __restrict__ gv, int64_t g_stride,
    double* __restrict__ div, int64_t d_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    const int nt = epb * pts;
    double* D = lds;
    double* X = D + NX * NX;
    double* Y = X + nt;
    double* Z = Y + nt;
    double* U = LDIM == 3 ? Z + nt : Z;      // the LDIM components of one vector, nt each
    const int tid = threadIdx.x;
    for (int t = tid; t < NX * NX; t += blockDim.x) D[t] = Dg[t];
    const TilePoint<LDIM, NX> q(D, tid, nt);
    const int le = tid / pts;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = tid < nt && e0 + le < nel;
        __syncthreads();
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
        }
        __syncthreads();
        double g[3][3], jacmi;
        geometric_factors<LDIM, NX>(q, X, Y, Z, g, jacmi);
        for (int v = 0; v < nvec; ++v) {
            if (v > 0) __syncthreads();   // every lane is done reading the previous vector
            if (live) {
#pragma unroll
                for (int d = 0; d < LDIM; ++d) U[d * nt + tid] = gv[((int64_t)v * LDIM + d) * g_stride + p];
            }
            __syncthreads();
            if (live) {
                double s = 0.0;
#pragma unroll
                for (int d = 0; d < LDIM; ++d) {
                    double ur, us, ut;
                    line_sums<LDIM, NX>(q, U + d * nt, ur, us, ut);
                    const double dd = physical_derivative<LDIM>(g, jacmi, d, ur, us, ut);
                    s = d == 0 ? dd : s + dd;
                }
                div[(int64_t)v * d_stride + p] = s;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// compute_dissipation's pointwise part (postproc.f90:784-796) and its glsc2 (:729), streaming:
//   dummy_c = re_c lap_re_c + im_c lap_im_c
//   diss    = ((0 + dummy_x) + dummy_y) [+ dummy_z];   diss = (0.5 diss) nu
//   s      += bm1 diss
// lap: 2 NC segments, the Re components then the Im components.  VEC: two points per thread by
// 16-byte loads (every base and stride even); the odd last point goes to one thread.
// ------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ double dissipation_at(const double (&re)[NC], const double (&im)[NC],
                                                 const double (&lr)[NC], const double (&li)[NC], double nu) {
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double dummy = re[c] * lr[c] + im[c] * li[c];
        s = s + dummy;
    }
    return 0.5 * s * nu;
}

template <int NC, bool VEC>
__global__ __launch_bounds__(kThreads) void k_pke_dissipation(int64_t n, const double* __restrict__ dRe,
                                                              const double* __restrict__ dIm, int64_t m_stride,
                                                              const double* __restrict__ lap, int64_t l_stride,
                                                              double nu, const double* __restrict__ bm1,
                                                              double* __restrict__ diss,
                                                              double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double lds4[4];
    double s = 0.0;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    auto point = [&](int64_t p) {
        double re[NC], im[NC], lr[NC], li[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            re[c] = dRe[c * m_stride + p];
            im[c] = dIm[c * m_stride + p];
            lr[c] = lap[c * l_stride + p];
            li[c] = lap[(NC + c) * l_stride + p];
        }
        const double v = dissipation_at<NC>(re, im, lr, li, nu);
        if (diss) diss[p] = v;
        s = s + bm1[p] * v;
    };
    if constexpr (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = t0; i < pairs; i += step) {
            const int64_t p = 2 * i;
            double rx[NC], ix[NC], lrx[NC], lix[NC], ry[NC], iy[NC], lry[NC], liy[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double2 a = ldq(dRe + c * m_stride + p), b = ldq(dIm + c * m_stride + p);
                const double2 e = ldq(lap + c * l_stride + p), f = ldq(lap + (NC + c) * l_stride + p);
                rx[c] = a.x, ry[c] = a.y, ix[c] = b.x, iy[c] = b.y;
                lrx[c] = e.x, lry[c] = e.y, lix[c] = f.x, liy[c] = f.y;
            }
            const double2 w = ld2(bm1 + p);
            const double2 v = make_double2(dissipation_at<NC>(rx, ix, lrx, lix, nu), dissipation_at<NC>(ry, iy, lry, liy, nu));
            if (diss) st2s(diss + p, v);
            s = s + w.x * v.x;
            s = s + w.y * v.y;
        }
        if ((n & 1) && t0 == 0) point(n - 1);
    } else {
        for (int64_t p = t0; p < n; p += step) point(p);
    }
    s = block_sum(s, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <int LDIM, int NX>
void launch_production(int64_t nel, const double* D, const double* xm, const double* ym, const double* zm,
                       const double* ubase, int64_t b_stride, const double* dRe, const double* dIm, int64_t m_stride,
                       const double* bm1, double* prod, int64_t p_stride, double* part, int grid, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)NX * NX + (size_t)2 * LDIM * epb * pts);
    static_assert(sizeof(double) * (10 * 10 + 2 * 3 * 1000) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    hipLaunchKernelGGL((k_pke_production<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D,
                       xm, ym, zm, ubase, b_stride, dRe, dIm, m_stride, bm1, prod, p_stride, part);
}

template <int LDIM, int NX>
void launch_divm1(int64_t nel, int nvec, const double* D, const double* xm, const double* ym, const double* zm,
                  const double* g, int64_t g_stride, double* div, int64_t d_stride, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)NX * NX + (size_t)2 * LDIM * epb * pts);
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 16384);
    hipLaunchKernelGGL((k_divm1<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, nvec, D, xm,
                       ym, zm, g, g_stride, div, d_stride);
}

}  // namespace

extern "C" {

int nkv_pke_production(const nkv_layout* L, int lx1, int ldim, const double* D, const double* xm, const double* ym,
                       const double* zm, const double* ubase, int64_t b_stride, const double* dRe, const double* dIm,
                       int64_t m_stride, const double* bm1, double* prod, int64_t p_stride, double* integrals_dev,
                       void* ws, void* stream) {
    static const char who[] = "pke_production";
    CHECK(check_layout(L));
    if (ldim != 2 && ldim != 3) return fail(NKV_EINVAL, "%s: ldim=%d must be 2 or 3", who, ldim);
    CHECK(need(integrals_dev, who, "integrals_dev"));
    CHECK(need(ws, who, "ws"));
    CHECK(check_ptr(ws, "ws"));
    hipStream_t st = S(stream);
    double* part = partials_of(ws);
    const int nq = ldim * ldim;
    if (L->n_v == 0)   // an empty shard: zeros, no other pointer is read
        return launch_reduce_cols(nq, part, 0, integrals_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
    CHECK(check_mesh_args(who, L, lx1, ldim, zm));
    if (b_stride < L->n_v || m_stride < L->n_v || (prod && p_stride < L->n_v))
        return fail(NKV_EINVAL, "%s: strides b_stride=%lld m_stride=%lld p_stride=%lld below n_v=%lld", who,
                    (long long)b_stride, (long long)m_stride, (long long)p_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(ubase, who, "ubase"));
    CHECK(need(dRe, who, "dRe"));
    CHECK(need(dIm, who, "dIm"));
    CHECK(need(bm1, who, "bm1"));
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    const int epb = tile_epb(pts);
    // one partial per term and workgroup: nq * grid <= 9 * NKV_MAXB slots, what nkv_workspace_bytes
    // guarantees from max_cols = 4 on; the grid is capped there and strides over the element groups
    const int grid = (int)std::min<int64_t>((nel + epb - 1) / epb, kMaxBlocks);
#define NKV_PP_PROD(NX)                                                                                          \
    case NX:                                                                                                     \
        if (ldim == 3)                                                                                           \
            launch_production<3, NX>(nel, D, xm, ym, zm, ubase, b_stride, dRe, dIm, m_stride, bm1, prod,        \
                                     p_stride, part, grid, st);                                                  \
        else                                                                                                     \
            launch_production<2, NX>(nel, D, xm, ym, zm, ubase, b_stride, dRe, dIm, m_stride, bm1, prod,        \
                                     p_stride, part, grid, st);                                                  \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_PP_PROD) }
#undef NKV_PP_PROD
    NKV_LAUNCHED();
    return launch_reduce_cols(nq, part, grid, integrals_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
}

int nkv_divm1(const nkv_layout* L, int lx1, int ldim, const double* D, const double* xm, const double* ym,
              const double* zm, const double* g, int nvec, int64_t g_stride, double* div, int64_t d_stride,
              void* stream) {
    static const char who[] = "divm1";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard (more ranks than elements): nothing to touch
    CHECK(check_mesh_args(who, L, lx1, ldim, zm));
    if (nvec < 1) return fail(NKV_EINVAL, "%s: nvec=%d < 1", who, nvec);
    if (g_stride < L->n_v || d_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: strides g_stride=%lld d_stride=%lld below n_v=%lld", who, (long long)g_stride,
                    (long long)d_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(g, who, "g"));
    CHECK(need(div, who, "div"));
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    hipStream_t st = S(stream);
#define NKV_PP_DIV(NX)                                                                                      \
    case NX:                                                                                                \
        if (ldim == 3) launch_divm1<3, NX>(nel, nvec, D, xm, ym, zm, g, g_stride, div, d_stride, st);      \
        else launch_divm1<2, NX>(nel, nvec, D, xm, ym, zm, g, g_stride, div, d_stride, st);                \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_PP_DIV) }
#undef NKV_PP_DIV
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pke_dissipation(const nkv_layout* L, const double* dRe, const double* dIm, int64_t m_stride,
                        const double* lap, int64_t l_stride, int ncomp, double nu, const double* bm1, double* diss,
                        double* integral_dev, void* ws, void* stream) {
    static const char who[] = "pke_dissipation";
    CHECK(check_layout(L));
    if (ncomp != 2 && ncomp != 3) return fail(NKV_EINVAL, "%s: ncomp=%d must be 2 or 3", who, ncomp);
    CHECK(need(integral_dev, who, "integral_dev"));
    CHECK(need(ws, who, "ws"));
    CHECK(check_ptr(ws, "ws"));
    hipStream_t st = S(stream);
    double* part = partials_of(ws);
    const int64_t n = L->n_v;
    if (n == 0)
        return launch_reduce_cols(1, part, 0, integral_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
    if (m_stride < n || l_stride < n)
        return fail(NKV_EINVAL, "%s: strides m_stride=%lld l_stride=%lld below n_v=%lld", who, (long long)m_stride,
                    (long long)l_stride, (long long)n);
    CHECK(need(dRe, who, "dRe"));
    CHECK(need(dIm, who, "dIm"));
    CHECK(need(lap, who, "lap"));
    CHECK(need(bm1, who, "bm1"));
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = a16(dRe) && a16(dIm) && a16(lap) && a16(bm1) && (!diss || a16(diss)) && m_stride % 2 == 0 &&
                     l_stride % 2 == 0 && n >= 2;
    const int grid = grid_for(vec ? n / 2 : n, kMaxBlocks);   // one partial per workgroup
    if (ncomp == 3) {
        if (vec)
            hipLaunchKernelGGL((k_pke_dissipation<3, true>), dim3(grid), dim3(kThreads), 0, st, n, dRe, dIm, m_stride, lap,
                               l_stride, nu, bm1, diss, part);
        else
            hipLaunchKernelGGL((k_pke_dissipation<3, false>), dim3(grid), dim3(kThreads), 0, st, n, dRe, dIm, m_stride, lap,
                               l_stride, nu, bm1, diss, part);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_pke_dissipation<2, true>), dim3(grid), dim3(kThreads), 0, st, n, dRe, dIm, m_stride, lap,
                               l_stride, nu, bm1, diss, part);
        else
            hipLaunchKernelGGL((k_pke_dissipation<2, false>), dim3(grid), dim3(kThreads), 0, st, n, dRe, dIm, m_stride, lap,
                               l_stride, nu, bm1, diss, part);
    }
    NKV_LAUNCHED();
    return launch_reduce_cols(1, part, grid, integral_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
}

}  // extern "C"
