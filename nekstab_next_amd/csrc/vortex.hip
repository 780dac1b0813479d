// vortex.hip — the flow-diagnostics layer on the device: the vortex criteria of vortex_core
// (postproc.f90:2-522) with their filter_s0 fused into one tiled pass over whole elements, the same
// filter as a standalone entry, and the component sums of nekStab_energy / nekStab_enstrophy
// (utils.f90:647-716).
//
// The reference forms the velocity-gradient tensor element by element (comp_gije), evaluates one
// criterion per call and filters the result with Nek5000's filter_s0; composed from the entries this
// library already had that is nkv_gradm1 (ldim^2 gradient fields written), a pointwise pass (read
// back) and a filter pass per criterion.  k_vortex_criteria stages the coordinates and the ldim
// velocity components once, keeps the tensor in registers, evaluates every selected criterion and
// runs the tensor-product filter in the LDS the coordinates no longer need: 2 ldim reads plus one
// write per criterion, per point.
#include "nkv_internal.h"

namespace {

constexpr unsigned bit_of(int code) { return 1u << code; }
constexpr unsigned kAllCriteria = (1u << NKV_VC_COUNT) - 1u;
// vorticity is stored raw (comp_vort3 averages it afterwards) and vortex_core calls lambda2 without
// filter_s0 (postproc.f90:8-9): neither is ever filtered
constexpr unsigned kFilterable = kAllCriteria & ~(bit_of(NKV_VC_VORTICITY) | bit_of(NKV_VC_LAMBDA2));

// ---- the invariants of the gradient tensor G[i][j] = du_i/dx_j (postproc.f90:346-435) ----------
template <int LDIM>
__device__ __forceinline__ double first_inv(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    if constexpr (LDIM == 3) return (G[0][0] + G[1][1]) + G[2][2];
    return G[0][0] + G[1][1];
}

template <int LDIM>
__device__ __forceinline__ double second_inv(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    if constexpr (LDIM == 3) {
        const double a = G[1][1] * G[2][2] - G[1][2] * G[2][1];
        const double b = G[0][0] * G[1][1] - G[0][1] * G[1][0];
        const double c = G[2][2] * G[0][0] - G[0][2] * G[2][0];
        return (a + b) + c;
    } else {   // :395-396 as written
        const double s = G[0][0] + G[1][1];
        double a = s * s;
        a = a - (2.0 * G[0][1]) * G[1][0];
        a = a - G[0][0] * G[0][0];
        a = a - G[1][1] * G[1][1];
        return a;
    }
}

template <int LDIM>
__device__ __forceinline__ double third_inv(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    if constexpr (LDIM == 3) {
        double a = -(G[0][0] * (G[1][2] * G[2][1] - G[1][1] * G[2][2]));
        a = a - G[0][1] * (G[1][0] * G[2][2] - G[2][0] * G[1][2]);
        a = a - G[0][2] * (G[2][0] * G[1][1] - G[1][0] * G[2][1]);
        return a;
    } else {
        return G[0][0] * G[1][1] - G[0][1] * G[1][0];
    }
}

// compute_delta (:198-205)
__device__ __forceinline__ double delta_of(double P1, double Q1, double R1) {
#pragma clang fp contract(off)
    const double Q = Q1 - (P1 * P1) / 3.0;
    double R = R1 + (((P1 * P1) * P1) * 2.0) / 27.0;
    R = R - (P1 * Q1) / 3.0;
    const double r2 = R / 2.0, q3 = Q / 3.0;
    return r2 * r2 + (q3 * q3) * q3;
}

// cubicLambdaCi (:437-474) with a = 1; sign(abs(r)**(1/3), r) is the real cube root
__device__ __forceinline__ double cubic_lambda_ci(double b, double c, double d) {
#pragma clang fp contract(off)
    const double f = c - (1.0 / 3.0) * (b * b);
    double g = 2.0 * ((b * b) * b);
    g = g - (9.0 * b) * c;
    g = g + 27.0 * d;
    g = g / 27.0;
    const double g2 = g / 2.0, f3 = f / 3.0;
    const double h = g2 * g2 + (f3 * f3) * f3;
    if (!(h > 0.0)) return h != h ? h : 0.0;   // h <= 0: no complex pair (a NaN stays a NaN)
    const double sh = sqrt(h);
    const double s = cbrt(-g2 + sh);
    const double u = cbrt(-g2 - sh);
    return ((s - u) * sqrt(3.0)) / 2.0;
}

// quadLambdaCi (:476-500) with a = 1
__device__ __forceinline__ double quad_lambda_ci(double b, double c) {
#pragma clang fp contract(off)
    const double d = b * b - 4.0 * c;
    if (d >= 0.0) return 0.0;
    return sqrt(fabs(d)) / 2.0;
}

// compute_omega_jc (:31-79): the sums of squares directly (i fastest, then j), not norm2()**2
template <int LDIM>
__device__ __forceinline__ double omega_of(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int j = 0; j < LDIM; ++j)
#pragma unroll
        for (int i = 0; i < LDIM; ++i) {
            const double ss = 0.5 * (G[i][j] + G[j][i]);
            const double oo = 0.5 * (G[i][j] - G[j][i]);
            sa = sa + ss * ss;
            sb = sb + oo * oo;
        }
    const double a = sa * sa, b = sb * sb;
    return b / ((a + b) + 1.0e-5);
}

// compute_antisymmetric (:307-325): the reference's '+' kept, so this is the off-diagonal strain
template <int LDIM>
__device__ __forceinline__ double assymetric_of(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    const double a = G[0][1] + G[1][0];
    if constexpr (LDIM == 3) {
        const double b = G[0][2] + G[2][0], c = G[1][2] + G[2][1];
        return ((a * a + b * b) + c * c) / 4.0;
    }
    return (a * a) / 4.0;
}

// compute_symmetric (:327-344)
template <int LDIM>
__device__ __forceinline__ double symmetric_of(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    const double B = assymetric_of<LDIM>(G);
    if constexpr (LDIM == 3) return B + ((G[0][0] * G[0][0] + G[1][1] * G[1][1]) + G[2][2] * G[2][2]) / 2.0;
    return B + (G[0][0] * G[0][0] + G[1][1] * G[1][1]) / 2.0;
}

// One Jacobi rotation of a symmetric 3 x 3 matrix annihilating a_pq (Rutishauser's formulas); r is the
// third index.  Branch-free: a_pq = 0 rotates by nothing.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
#pragma clang fp contract(off)
    const bool nz = apq != 0.0;
    const double den = nz ? apq : 1.0;
    const double theta = (aqq - app) / (2.0 * den);
    double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = nz ? t : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0 * apq;
    const double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
}

// lambda2 (Nek5000's; Jeong & Hussain): the middle eigenvalue of A = S^2 + O^2.  The trigonometric closed
// form loses half the digits at a double eigenvalue (acos near +-1), which is exactly a solid-body
// rotation (A = diag(-W^2, -W^2, 0): 5.7e-9 relative), so the eigenvalues come from five cyclic Jacobi
// sweeps over (0,1), (0,2), (1,2): + - * / sqrt only, in a fixed order, a few eps of ||A|| everywhere.
constexpr int kJacobiSweeps = 5;
__device__ __forceinline__ double lambda2_of(const double (&G)[3][3]) {
#pragma clang fp contract(off)
    double S[3][3], O[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            S[i][j] = 0.5 * (G[i][j] + G[j][i]);
            O[i][j] = 0.5 * (G[i][j] - G[j][i]);
        }
    auto entry = [&](int i, int j) {
        double acc = S[i][0] * S[0][j];
        acc = acc + O[i][0] * O[0][j];
#pragma unroll
        for (int k = 1; k < 3; ++k) {
            acc = acc + S[i][k] * S[k][j];
            acc = acc + O[i][k] * O[k][j];
        }
        return acc;
    };
    double a00 = entry(0, 0), a01 = entry(0, 1), a02 = entry(0, 2);
    double a11 = entry(1, 1), a12 = entry(1, 2), a22 = entry(2, 2);
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12);
        jacobi_rotate(a00, a22, a02, a01, a12);
        jacobi_rotate(a11, a22, a12, a01, a02);
    }
    const double lo = a00 < a11 ? a00 : a11, hi = a00 < a11 ? a11 : a00;
    const double m = hi < a22 ? hi : a22;
    return lo > m ? lo : m;
}

// ------------------------------------------------------------------------------------------
// Nek5000's filter_s0 / filterq on one staged field: v <- F v along r, then s, then t
//   v'(i,j,k) = sum_m F[i][m] v(m,j,k)     (m ascending, products not contracted)
// P, Q: two scratch tiles (nt doubles each).  Every lane of the workgroup must call it (barriers);
// `owns`: the lane holds a live point.  In 3-D P and Q come back swapped, so the next call writes
// the tile nobody still reads.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__device__ __forceinline__ double filter_point(const TilePoint<LDIM, NX>& q, const double* Fi, const double* Fj,
                                               const double* Fk, double*& P, double*& Q, int tid, bool owns,
                                               double v) {
#pragma clang fp contract(off)
    constexpr int sj = NX, sk = NX * NX;
    if (owns) P[tid] = v;
    __syncthreads();
    double a = Fi[0] * P[q.ri];
#pragma unroll 2
    for (int m = 1; m < NX; ++m) a = a + Fi[m] * P[q.ri + m];
    if (owns) Q[tid] = a;
    __syncthreads();
    double b = Fj[0] * Q[q.si];
#pragma unroll 2
    for (int m = 1; m < NX; ++m) b = b + Fj[m] * Q[q.si + m * sj];
    if constexpr (LDIM == 2) {
        return b;   // the next call's write of P is fenced from this call's reads of P by the barrier above
    } else {
        if (owns) P[tid] = b;
        __syncthreads();
        double c = Fk[0] * P[q.ti];
#pragma unroll 2
        for (int m = 1; m < NX; ++m) c = c + Fk[m] * P[q.ti + m * sk];
        double* t = P;
        P = Q;
        Q = t;
        return c;
    }
}

// ------------------------------------------------------------------------------------------
// The fused pass.  LDS: D, F (NX*NX each), X, Y, [Z], U[LDIM] (nt each); once the geometric factors
// and the tensor are in registers, X and Y are the filter's scratch tiles.
// ------------------------------------------------------------------------------------------
// Occupancy, as for k_pke_production: the tensor and the criteria on top of k_gradm1's registers come to
// 157 VGPRs at lx1 = 8 in 3-D (three waves per SIMD: ONE 512-thread workgroup per CU); asking for four
// waves per SIMD (128 VGPRs) fits two.  Workgroups above 512 threads (lx1 = 9, 10) keep the default.
template <int LDIM, int NX>
constexpr int criteria_min_waves() { return tile_threads<LDIM, NX>() <= 512 ? 4 : 0; }

template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>()), (criteria_min_waves<LDIM, NX>())) void k_vortex_criteria(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ Fg, const double* __restrict__ xm,
    const double* __restrict__ ym, const double* __restrict__ zm, const double* __restrict__ u, int64_t u_stride,
    unsigned mask, unsigned fmask, double* __restrict__ out, int64_t o_stride, double* __restrict__ grad,
    int64_t g_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    const int nt = epb * pts;
    double* D = lds;                         // D(i, m) at D[i*NX + m]
    double* F = D + NX * NX;                 // F(i, m) likewise
    double* X = F + NX * NX;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    double* U = LDIM == 3 ? Z + nt : Z;      // LDIM velocity components, nt each
    const int tid = threadIdx.x;
    for (int t = tid; t < NX * NX; t += blockDim.x) {
        D[t] = Dg[t];
        if (fmask) F[t] = Fg[t];
    }
    const TilePoint<LDIM, NX> q(D, tid, nt);
    const double *Fi = q.Di + NX * NX, *Fj = q.Dj + NX * NX, *Fk = q.Dk + NX * NX;
    const int le = tid / pts;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = tid < nt && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and D, F are staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
#pragma unroll
            for (int c = 0; c < LDIM; ++c) U[c * nt + tid] = u[c * u_stride + p];
        }
        __syncthreads();
        double gf[3][3], jacmi;   // dead lanes compute garbage they never store
        geometric_factors<LDIM, NX>(q, X, Y, Z, gf, jacmi);
        double G[3][3];
#pragma unroll
        for (int c = 0; c < LDIM; ++c) {
            double ur, us, ut;
            line_sums<LDIM, NX>(q, U + c * nt, ur, us, ut);
#pragma unroll
            for (int d = 0; d < LDIM; ++d) G[c][d] = physical_derivative<LDIM>(gf, jacmi, d, ur, us, ut);
        }
        if (grad && live) {
#pragma unroll
            for (int c = 0; c < LDIM; ++c)
#pragma unroll
                for (int d = 0; d < LDIM; ++d) grad[(int64_t)(c * LDIM + d) * g_stride + p] = G[c][d];
        }
        if (fmask) __syncthreads();   // every lane has its factors: X and Y turn into filter scratch
        double *P = X, *Q = Y;
        int slot = 0;
        auto emit = [&](int code, double v) {   // mask and fmask are uniform: so are the barriers inside
            if (fmask & bit_of(code)) v = filter_point<LDIM, NX>(q, Fi, Fj, Fk, P, Q, tid, live, v);
            if (code == NKV_VC_SWIRLING) v = v * v;   // :298-302, after the filter
            if (live) out[(int64_t)slot * o_stride + p] = v;
            ++slot;
        };
        if (mask & bit_of(NKV_VC_VORTICITY)) {
            if constexpr (LDIM == 3) {
                emit(NKV_VC_VORTICITY, G[2][1] - G[1][2]);
                emit(NKV_VC_VORTICITY, G[0][2] - G[2][0]);
            }
            emit(NKV_VC_VORTICITY, G[1][0] - G[0][1]);
        }
        if constexpr (LDIM == 3) {
            if (mask & bit_of(NKV_VC_LAMBDA2)) emit(NKV_VC_LAMBDA2, lambda2_of(G));
        }
        if (mask & bit_of(NKV_VC_Q)) emit(NKV_VC_Q, second_inv<LDIM>(G));
        if (mask & bit_of(NKV_VC_DELTA))
            emit(NKV_VC_DELTA, delta_of(-first_inv<LDIM>(G), second_inv<LDIM>(G), -third_inv<LDIM>(G)));
        double lci = 0.0;   // cubicLambdaCi (3-D) / quadLambdaCi (2-D), shared by swirling and lambda_ci
        if (mask & (bit_of(NKV_VC_SWIRLING) | bit_of(NKV_VC_LAMBDA_CI))) {
            if constexpr (LDIM == 3)
                lci = cubic_lambda_ci(-first_inv<LDIM>(G), second_inv<LDIM>(G), -third_inv<LDIM>(G));
            else
                lci = quad_lambda_ci(-first_inv<LDIM>(G), -third_inv<LDIM>(G));
        }
        if (mask & bit_of(NKV_VC_SWIRLING)) emit(NKV_VC_SWIRLING, lci);
        if (mask & bit_of(NKV_VC_OMEGA)) emit(NKV_VC_OMEGA, omega_of<LDIM>(G));
        if (mask & bit_of(NKV_VC_SYMMETRIC)) emit(NKV_VC_SYMMETRIC, symmetric_of<LDIM>(G));
        if (mask & bit_of(NKV_VC_ASSYMETRIC)) emit(NKV_VC_ASSYMETRIC, assymetric_of<LDIM>(G));
        if (mask & bit_of(NKV_VC_LAMBDA_CI)) emit(NKV_VC_LAMBDA_CI, lci);
    }
}

// The same filter on nfld fields (field f at v + f v_stride -> out + f o_stride; out may be v).
// LDS: F, then two scratch tiles.
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_filter_s0(int64_t nel, int epb, int nfld,
                                                                         const double* __restrict__ Fg,
                                                                         const double* v, int64_t v_stride,
                                                                         double* out, int64_t o_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    const int nt = epb * pts;
    double* F = lds;
    double* P = F + NX * NX;
    double* Q = P + nt;
    const int tid = threadIdx.x;
    for (int t = tid; t < NX * NX; t += blockDim.x) F[t] = Fg[t];
    const TilePoint<LDIM, NX> q(F, tid, nt);   // its rows of "D" are this point's rows of F
    const int le = tid / pts;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = tid < nt && e0 + le < nel;
        for (int f = 0; f < nfld; ++f) {
            __syncthreads();   // the previous field's (group's) reads are done (and F is staged)
            const double x = live ? v[(int64_t)f * v_stride + p] : 0.0;
            const double y = filter_point<LDIM, NX>(q, q.Di, q.Dj, q.Dk, P, Q, tid, live, x);
            if (live) out[(int64_t)f * o_stride + p] = y;
        }
    }
}

// ------------------------------------------------------------------------------------------
// nekStab_energy / nekStab_enstrophy's sums (utils.f90:671-674, 708-710), one streaming pass:
//   s_c += f_c w f_c  (glsc3's operand order), c < NC;   s_3 += t w y  (pot, :674) when t is given
// partials[q * gridDim.x + block], q < 4.  VEC: two points per thread by 16-byte loads.
// ------------------------------------------------------------------------------------------
template <int NC, bool VEC>
__global__ __launch_bounds__(kThreads) void k_energy_components(int64_t n, const double* __restrict__ w,
                                                                const double* __restrict__ f, int64_t f_stride,
                                                                const double* __restrict__ t,
                                                                const double* __restrict__ y,
                                                                double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double red[4][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    auto point = [&](int64_t p) {
        const double wp = w[p];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double fc = f[c * f_stride + p];
            s[c] = s[c] + (fc * wp) * fc;
        }
        if (t) s[3] = s[3] + (t[p] * wp) * y[p];
    };
    if constexpr (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = t0; i < pairs; i += step) {
            const int64_t p = 2 * i;
            const double2 wp = ld2(w + p);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double2 fc = ldq(f + c * f_stride + p);
                s[c] = s[c] + (fc.x * wp.x) * fc.x;
                s[c] = s[c] + (fc.y * wp.y) * fc.y;
            }
            if (t) {
                const double2 tp = ldq(t + p), yp = ld2(y + p);
                s[3] = s[3] + (tp.x * wp.x) * yp.x;
                s[3] = s[3] + (tp.y * wp.y) * yp.y;
            }
        }
        if ((n & 1) && t0 == 0) point(n - 1);
    } else {
        for (int64_t p = t0; p < n; p += step) point(p);
    }
    // fixed-order block reduction: lanes of a wave, then the four waves in ascending order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double v = wave_sum(s[c]);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double r = 0.0;
        for (int wv = 0; wv < 4; ++wv) r = r + red[wv][threadIdx.x];
        partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
    }
}

template <int LDIM, int NX>
void launch_criteria(int64_t nel, const double* D, const double* F, const double* xm, const double* ym,
                     const double* zm, const double* u, int64_t u_stride, unsigned mask, unsigned fmask, double* out,
                     int64_t o_stride, double* grad, int64_t g_stride, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)2 * NX * NX + (size_t)2 * LDIM * epb * pts);
    static_assert(sizeof(double) * (2 * 10 * 10 + 2 * 3 * 1000) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 16384);
    hipLaunchKernelGGL((k_vortex_criteria<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D, F,
                       xm, ym, zm, u, u_stride, mask, fmask, out, o_stride, grad, g_stride);
}

template <int LDIM, int NX>
void launch_filter(int64_t nel, int nfld, const double* F, const double* v, int64_t v_stride, double* out,
                   int64_t o_stride, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)NX * NX + (size_t)2 * epb * pts);
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 16384);
    hipLaunchKernelGGL((k_filter_s0<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, nfld, F, v,
                       v_stride, out, o_stride);
}

}  // namespace

extern "C" {

int nkv_vortex_criteria(const nkv_layout* L, int lx1, int ldim, const double* D, const double* F, const double* xm,
                        const double* ym, const double* zm, const double* u, int64_t u_stride, unsigned mask,
                        unsigned filter_mask, double* out, int64_t o_stride, double* grad, int64_t g_stride,
                        void* stream) {
    static const char who[] = "vortex_criteria";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch
    CHECK(check_mesh_args(who, L, lx1, ldim, zm));
    if (mask & ~kAllCriteria) return fail(NKV_EINVAL, "%s: mask=0x%x has bits beyond the %d criteria", who, mask, NKV_VC_COUNT);
    if (filter_mask & ~kAllCriteria)
        return fail(NKV_EINVAL, "%s: filter_mask=0x%x has bits beyond the %d criteria", who, filter_mask, NKV_VC_COUNT);
    if (!mask && !grad) return fail(NKV_EINVAL, "%s: mask=0 selects no criterion and grad is NULL", who);
    if (ldim == 2 && (mask & bit_of(NKV_VC_LAMBDA2)))
        return fail(NKV_EINVAL, "%s: lambda2 is 3-D only (ldim=%d)", who, ldim);
    if (F && lx1 < 3) return fail(NKV_EINVAL, "%s: lx1=%d < 3 has no mode to filter", who, lx1);
    if (u_stride < L->n_v) return fail(NKV_EINVAL, "%s: u_stride=%lld below n_v=%lld", who, (long long)u_stride, (long long)L->n_v);
    if (mask && o_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: o_stride=%lld below n_v=%lld", who, (long long)o_stride, (long long)L->n_v);
    if (grad && g_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: g_stride=%lld below n_v=%lld", who, (long long)g_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(u, who, "u"));
    if (mask) CHECK(need(out, who, "out"));
    const unsigned fmask = F ? (mask & filter_mask & kFilterable) : 0u;
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    hipStream_t st = S(stream);
#define NKV_VX_CRIT(NX)                                                                                          \
    case NX:                                                                                                     \
        if (ldim == 3)                                                                                           \
            launch_criteria<3, NX>(nel, D, F, xm, ym, zm, u, u_stride, mask, fmask, out, o_stride, grad,        \
                                   g_stride, st);                                                                \
        else                                                                                                     \
            launch_criteria<2, NX>(nel, D, F, xm, ym, zm, u, u_stride, mask, fmask, out, o_stride, grad,        \
                                   g_stride, st);                                                                \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_VX_CRIT) }
#undef NKV_VX_CRIT
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_filter_s0(const nkv_layout* L, int lx1, int ldim, const double* F, const double* v, int64_t v_stride,
                  int nfld, double* out, int64_t o_stride, void* stream) {
    static const char who[] = "filter_s0";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;
    if (ldim != 2 && ldim != 3) return fail(NKV_EINVAL, "%s: ldim=%d must be 2 or 3", who, ldim);
    if (lx1 < 3 || lx1 > 10) return fail(NKV_EINVAL, "%s: lx1=%d outside 3..10", who, lx1);
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    if (L->n_v % pts != 0)
        return fail(NKV_EINVAL, "%s: %d points per element (lx1=%d) do not divide n_v=%lld", who, pts, lx1,
                    (long long)L->n_v);
    if (nfld < 1) return fail(NKV_EINVAL, "%s: nfld=%d < 1", who, nfld);
    if (v_stride < L->n_v) return fail(NKV_EINVAL, "%s: v_stride=%lld below n_v=%lld", who, (long long)v_stride, (long long)L->n_v);
    if (o_stride < L->n_v) return fail(NKV_EINVAL, "%s: o_stride=%lld below n_v=%lld", who, (long long)o_stride, (long long)L->n_v);
    CHECK(need(F, who, "F"));
    CHECK(need(v, who, "v"));
    CHECK(need(out, who, "out"));
    const int64_t nel = L->n_v / pts;
    hipStream_t st = S(stream);
#define NKV_VX_FILT(NX)                                                                          \
    case NX:                                                                                     \
        if (ldim == 3) launch_filter<3, NX>(nel, nfld, F, v, v_stride, out, o_stride, st);       \
        else launch_filter<2, NX>(nel, nfld, F, v, v_stride, out, o_stride, st);                 \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_VX_FILT) }
#undef NKV_VX_FILT
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_energy_components(const nkv_layout* L, const double* w, const double* f, int64_t f_stride, int ncomp,
                          const double* t, const double* y, double* sums_dev, void* ws, void* stream) {
    static const char who[] = "energy_components";
    CHECK(check_layout(L));
    if (ncomp < 1 || ncomp > 3) return fail(NKV_EINVAL, "%s: ncomp=%d outside 1..3", who, ncomp);
    CHECK(need(sums_dev, who, "sums_dev"));
    CHECK(need(ws, who, "ws"));
    CHECK(check_ptr(ws, "ws"));
    hipStream_t st = S(stream);
    double* part = partials_of(ws);
    const int64_t n = L->n_v;
    if (n == 0)   // an empty shard: four zeros, no other pointer is read
        return launch_reduce_cols(4, part, 0, sums_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
    if (f_stride < n) return fail(NKV_EINVAL, "%s: f_stride=%lld below n_v=%lld", who, (long long)f_stride, (long long)n);
    CHECK(need(w, who, "w"));
    CHECK(need(f, who, "f"));
    if ((t != nullptr) != (y != nullptr)) return fail(NKV_EINVAL, "%s: t and y must be given together", who);
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = a16(w) && a16(f) && f_stride % 2 == 0 && (!t || (a16(t) && a16(y))) && n >= 2;
    const int grid = grid_for(vec ? n / 2 : n, kMaxBlocks);   // four partials per workgroup
#define NKV_VX_EN(NC)                                                                                               \
    case NC:                                                                                                        \
        if (vec)                                                                                                    \
            hipLaunchKernelGGL((k_energy_components<NC, true>), dim3(grid), dim3(kThreads), 0, st, n, w, f, f_stride, t, \
                               y, part);                                                                            \
        else                                                                                                        \
            hipLaunchKernelGGL((k_energy_components<NC, false>), dim3(grid), dim3(kThreads), 0, st, n, w, f, f_stride, t, \
                               y, part);                                                                            \
        break;
    switch (ncomp) { NKV_VX_EN(1) NKV_VX_EN(2) NKV_VX_EN(3) }
#undef NKV_VX_EN
    NKV_LAUNCHED();
    return launch_reduce_cols(4, part, grid, sums_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
}

}  // extern "C"
