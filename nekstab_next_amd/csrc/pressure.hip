// pressure.hip — the P_N - P_{N-2} pressure operators of an incompressible flow on the GLL mesh and the fused
// conjugate-gradient iteration of the divergence-free projection behind pressure.DivergenceFreeProjector
// (Nek5000's opdiv / opgradt / cdabdtp, navier1.f).  Notation of advdiff.hip: g[d][a] the cofactors of
// k_gradm1 (geometric_factors_jac), D_a the GLL line derivative; lx2 = lx1 - 2 Gauss-Legendre points per
// direction carry the pressure, I (lx2 x lx1) interpolates from the GLL to the Gauss points, I^ is its tensor
// product and w^ the tensor product of the Gauss weights.  The pressure is element-discontinuous
// (nel lx2^ldim values), nothing on its mesh is assembled.
//   k_pressure_div:    (D u)[e,q]  = w^_q I^( sum_{d<ldim} sum_a g[d][a] D_a (m u_d) )[e,q]      (m: optional)
//   k_pressure_gradt:  (D^T p)_d   = sum_a D_a^T [ g[d][a] I^^T(w^ p) ]                         (unassembled)
// two matrices that are transposes of each other.  Both tile like k_advdiff_rhs (whole elements per workgroup,
// one GLL point per thread, factors formed once per group) and interpolate by sum factorisation, one direction
// at a time through LDS.  No atomics, no contraction; element-local, so any element sub-range gives the bits
// of the whole.
// With E = D minv dsavg D^T the iteration of unpreconditioned CG on E (or on Z E Z, Z = I - 1 1^T / n, when
// the constant is a null vector) is three launches and one dsavg batch:
//   k_pressure_gradt      forms p = r + beta p on its load (beta from the partials of r.r) and writes D^T p
//   k_pressure_div        applies minv on its load and emits the partials of p.Ep, sum Ep and sum p
//   k_pressure_cg_update  alpha from those partials; x += alpha p, r -= alpha (Ep - mean Ep); partials of r.r
// Every scalar stays on the device: a producer writes one partial per workgroup into a fixed slot, and every
// workgroup of the consumer sums the slots in the same fixed order (cg_scalar), so all of them hold the same
// bits and the same input gives the same bits run to run.
// k_pressure_div2, k_pressure_gradt2 and k_pressure_cg_update2 run that iteration for two systems on one mesh (the
// re and the im half of a pair vector: the projection inside a stage of the incompressible resolvent) in one launch
// each, with the bits of the single-system kernels for either system; they stand behind the kernels above.
// k_pressure_precond applies the fast-diagonalisation preconditioner M of pressure.py (its comment below), and the
// preconditioned iteration  z = Z M r,  p = z + (r.z / r.z_prev) p,  alpha = r.z / p.(Z E p)  is four launches:
//   k_pressure_gradt      with zsum: p = (z - zeta) + beta p on its load, zeta = sum z / n, beta from the partials of r.z
//   k_pressure_div        as above
//   k_pressure_cg_update  as above, given the partials of r.z for those of r.r; it emits r.r for the stop rule
//   k_pressure_precond    z = M r; partials of r.z and sum z
// The apply is its own kernel behind the update, not a rider in an element-tiled update: the update keeps its
// streaming rate and its bits, the apply also serves DivergenceFreeProjector.precondition, and what riding would
// save is the second read of r.  Per iteration, in doubles (n GLL points, m pressure values, ldim = 3):
// gradt 6 n + 3 m, div 7 n + 2 m, update 6 m, precond 2 m: 13 n + 13 m against 13 n + 11 m unpreconditioned
// (1.672 GB against 1.596 GB at lx1 = 8, E = 22,088), plus the dsavg batch either way.
#include "nkv_internal.h"

namespace {

constexpr int kPB = NKV_PRESSURE_PARTIALS;   // partial slots per reduced quantity
static_assert(kPB % 64 == 0, "cg_scalar strides the slots by one wave");

// The sum of B partials in a fixed order, the same bits in every workgroup of every kernel that calls it:
// the first wave strides over the slots, then a fixed exchange pattern.  Every thread of the block returns
// the sum.  slot: one LDS double per call site.
__device__ __forceinline__ double cg_scalar(const double* __restrict__ part, int B, double* slot) {
    if (threadIdx.x < 64) {
        double s = 0.0;
        for (int b = threadIdx.x; b < B; b += 64) s += part[b];
        s = wave_sum(s);
        if (threadIdx.x == 0) *slot = s;
    }
    __syncthreads();
    return *slot;
}

// Block-wide sums of three per-thread values (whole waves, up to kMaxWaves): waves in ascending order.
// Valid in thread 0.  red: 3 * kMaxWaves doubles of LDS.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) {
        red[wave] = a;
        red[kMaxWaves + wave] = b;
        red[2 * kMaxWaves + wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0];
        b = red[kMaxWaves];
        c = red[2 * kMaxWaves];
        for (int w = 1; w < nw; ++w) {
            a += red[w];
            b += red[kMaxWaves + w];
            c += red[2 * kMaxWaves + w];
        }
    }
}

// The head of the LDS both tiled kernels carve: D, the interpolation matrix, the Gauss weights and the
// reduction scratch (an even number of doubles: the tiles behind it stay 16-byte aligned).
template <int NX>
constexpr int head_doubles() {
    return NX * NX + (NX - 2) * NX + (NX - 2) + (NX & 1) + 3 * kMaxWaves + 2;
}
template <int LDIM, int NX>
constexpr int pressure_pts() { return LDIM == 3 ? (NX - 2) * (NX - 2) * (NX - 2) : (NX - 2) * (NX - 2); }

template <int NX>
struct Head {
    double *D, *I, *gw, *red, *tiles;
    __device__ __forceinline__ Head(double* lds, const double* Dg, const double* Ig, const double* gwg) {
        constexpr int M = NX - 2;
        D = lds;
        I = D + NX * NX;        // I(q, i) at I[q*NX + i]
        gw = I + M * NX;
        red = gw + M + (NX & 1);
        tiles = lds + head_doubles<NX>();
        for (int t = threadIdx.x; t < NX * NX; t += blockDim.x) D[t] = Dg[t];
        for (int t = threadIdx.x; t < M * NX; t += blockDim.x) I[t] = Ig[t];
        for (int t = threadIdx.x; t < M; t += blockDim.x) gw[t] = gwg[t];
    }
};

// ------------------------------------------------------------------------------------------
// The weak divergence on the pressure mesh.  Per element group: stage the coordinates, form the factors,
// stage the ldim velocity components over the coordinate tiles (times m when given), take the line sums
//   dv = sum_d (g[d][0] u_d,r + g[d][1] u_d,s [+ g[d][2] u_d,t])          (jac div u at the GLL point)
// and interpolate dv to the Gauss points along r, then s[, then t], ping-pong between two of the tiles; the
// thread that owns Gauss point q of its element scales by w^_q and stores.  With pv given the same thread
// accumulates pv.out, sum out and sum pv, and the workgroup writes the three partials into its slots.
// LDS: head + ldim nt doubles.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_pressure_div(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ Ig, const double* __restrict__ gwg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ u, int64_t u_stride, const double* __restrict__ mult, double* __restrict__ out,
    const double* __restrict__ pv, double* __restrict__ partials) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int M = NX - 2;
    constexpr int ppts = pressure_pts<LDIM, NX>();
    const int nt = epb * pts;
    const Head<NX> h(lds, Dg, Ig, gwg);
    const double* I = h.I;
    double* X = h.tiles;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    const int tid = threadIdx.x;
    const TilePoint<LDIM, NX> q(h.D, tid, nt);
    const int le = tid / pts, rr = tid - le * pts;
    const int eb = le * pts;                 // this thread's element inside the tiles (used below tid < nt only)
    const bool intile = tid < nt;
    double s_pe = 0.0, s_e = 0.0, s_p = 0.0;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = intile && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and the head is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
        }
        __syncthreads();
        double g[3][3], jac;   // dead lanes compute garbage they never store
        geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
        __syncthreads();       // every lane has formed its factors: the tiles are free
        if (live) {
            const double m = mult ? mult[p] : 1.0;
            double* tiles[3] = {X, Y, Z};
#pragma unroll
            for (int d = 0; d < LDIM; ++d) {
                const double v = u[d * u_stride + p];
                tiles[d][tid] = mult ? m * v : v;
            }
        }
        __syncthreads();
        double dv = 0.0;
        {
            const double* tiles[3] = {X, Y, Z};
#pragma unroll
            for (int d = 0; d < LDIM; ++d) {
                double ur, us, ut;
                line_sums<LDIM, NX>(q, tiles[d], ur, us, ut);
                double t = g[d][0] * ur + g[d][1] * us;
                if constexpr (LDIM == 3) t = t + g[d][2] * ut;
                dv = d == 0 ? t : dv + t;
            }
        }
        __syncthreads();       // the velocity tiles are read
        if (intile) X[tid] = dv;
        __syncthreads();
        // along r: X(i, j, k) -> Y(a, j, k), a < M
        constexpr int n1 = LDIM == 3 ? M * NX * NX : M * NX;
        if (intile && rr < n1) {
            const int a = rr % M, row = rr / M;          // row = j + NX k
            const double* src = X + eb + row * NX;
            double acc = I[a * NX] * src[0];
#pragma unroll 2
            for (int m = 1; m < NX; ++m) acc = acc + I[a * NX + m] * src[m];
            Y[eb + rr] = acc;
        }
        __syncthreads();
        // along s: Y(a, j, k) -> (a, b, k)
        constexpr int n2 = LDIM == 3 ? M * M * NX : M * M;
        double val = 0.0;
        if (intile && rr < n2) {
            const int a = rr % M, b = (rr / M) % M, k = rr / (M * M);
            const double* src = Y + eb + a + M * NX * k;
            double acc = I[b * NX] * src[0];
#pragma unroll 2
            for (int m = 1; m < NX; ++m) acc = acc + I[b * NX + m] * src[M * m];
            if constexpr (LDIM == 3) X[eb + rr] = acc;
            val = acc;
        }
        if constexpr (LDIM == 3) {
            __syncthreads();
            // along t: X(a, b, k) -> (a, b, c)
            if (intile && rr < ppts) {
                const int c = rr / (M * M), ab = rr - c * M * M;
                const double* src = X + eb + ab;
                double acc = I[c * NX] * src[0];
#pragma unroll 2
                for (int m = 1; m < NX; ++m) acc = acc + I[c * NX + m] * src[M * M * m];
                val = acc;
            }
        }
        if (live && rr < ppts) {
            const int a = rr % M, b = (rr / M) % M, c = LDIM == 3 ? rr / (M * M) : 0;
            const double wab = h.gw[a] * h.gw[b];
            const double wq = LDIM == 3 ? wab * h.gw[c] : wab;
            const double o = wq * val;
            const int64_t pp = (e0 + le) * ppts + rr;
            out[pp] = o;
            if (pv) {
                const double pe = pv[pp];
                s_pe += pe * o;
                s_e += o;
                s_p += pe;
            }
        }
    }
    if (partials) {
        block_sum3(s_pe, s_e, s_p, h.red);
        if (tid == 0) {
            partials[blockIdx.x] = s_pe;
            partials[kPB + blockIdx.x] = s_e;
            partials[2 * kPB + blockIdx.x] = s_p;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The transposed operator.  Per element group: stage the coordinates and, by the thread that owns Gauss point
// q, w^_q p_q (with res given, p <- first ? res : res + beta p is formed here and stored back, beta =
// rr_new / rr_old from the partials); interpolate transposed along t[, then s], then r back to the GLL points
// (the factors are formed meanwhile); then for every direction d write the fluxes g[d][a] s over the
// coordinate tiles and take the transposed line sums of k_advdiff_rhs.  LDS: head + (ldim + 2) nt doubles,
// 41,904 bytes at lx1 = 10 in 3-D.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_pressure_gradt(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ Ig, const double* __restrict__ gwg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm, double* pin,
    const double* __restrict__ res, const double* __restrict__ rr_new, const double* __restrict__ rr_old, int B,
    int first, double* __restrict__ t, int64_t t_stride, const double* __restrict__ zsum, double inv_n) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int M = NX - 2;
    constexpr int ppts = pressure_pts<LDIM, NX>();
    const int nt = epb * pts;
    const Head<NX> h(lds, Dg, Ig, gwg);
    const double* I = h.I;
    double* X = h.tiles;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    double* A = LDIM == 3 ? Z + nt : Z;
    double* Bt = A + nt;
    const int tid = threadIdx.x;
    double beta = 0.0;
    if (res && !first) {   // (uniform over the grid)
        const double num = cg_scalar(rr_new, B, h.red), den = cg_scalar(rr_old, B, h.red + 1);
        beta = den != 0.0 ? num / den : 0.0;
    }
    // the preconditioned iteration: res is M r, whose mean leaves here (zeta = sum z / n; uniform over the grid)
    const double zeta = res && zsum ? cg_scalar(zsum, B, h.red + 2) * inv_n : 0.0;
    const TilePoint<LDIM, NX> q(h.D, tid, nt);
    const int le = tid / pts, rr = tid - le * pts;
    const int eb = le * pts;
    const bool intile = tid < nt;
    const int pi = q.i;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = intile && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and the head is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
            if (rr < ppts) {
                const int a = rr % M, b = (rr / M) % M, c = LDIM == 3 ? rr / (M * M) : 0;
                const double wab = h.gw[a] * h.gw[b];
                const double wq = LDIM == 3 ? wab * h.gw[c] : wab;
                const int64_t pp = (e0 + le) * ppts + rr;
                double v;
                if (res) {
                    double rv = res[pp];
                    if (zsum) rv = rv - zeta;
                    v = first ? rv : rv + beta * pin[pp];
                    pin[pp] = v;
                } else {
                    v = pin[pp];
                }
                A[eb + rr] = wq * v;
            }
        }
        __syncthreads();
        double g[3][3], jac;   // dead lanes compute garbage they never store
        geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
        double* S1 = A;        // the tile the transposed s pass reads
        double* S2 = Bt;       // ... and writes
        if constexpr (LDIM == 3) {
            // along t, transposed: A(a, b, c) -> Bt(a, b, k)
            if (intile && rr < M * M * NX) {
                const int k = rr / (M * M), ab = rr - k * M * M;
                const double* src = A + eb + ab;
                double acc = I[k] * src[0];
#pragma unroll 2
                for (int c = 1; c < M; ++c) acc = acc + I[c * NX + k] * src[M * M * c];
                Bt[eb + rr] = acc;
            }
            __syncthreads();
            S1 = Bt;
            S2 = A;
        }
        // along s, transposed: S1(a, b, k) -> S2(a, j, k)
        constexpr int n2 = LDIM == 3 ? M * NX * NX : M * NX;
        if (intile && rr < n2) {
            const int a = rr % M, j = (rr / M) % NX, k = rr / (M * NX);
            const double* src = S1 + eb + a + M * M * k;
            double acc = I[j] * src[0];
#pragma unroll 2
            for (int b = 1; b < M; ++b) acc = acc + I[b * NX + j] * src[M * b];
            S2[eb + rr] = acc;
        }
        __syncthreads();
        // along r, transposed: S2(a, j, k) -> the GLL point (i, j, k)
        double s = 0.0;
        if (intile) {
            const double* src = S2 + eb + M * (rr / NX);
            s = I[pi] * src[0];
#pragma unroll 2
            for (int a = 1; a < M; ++a) s = s + I[a * NX + pi] * src[a];
        }
        // (every lane formed its factors before the barriers above: the coordinate tiles are free)
#pragma unroll
        for (int d = 0; d < LDIM; ++d) {
            if (d > 0) __syncthreads();   // the previous direction's fluxes are read
            if (intile) {
                X[tid] = g[d][0] * s;
                Y[tid] = g[d][1] * s;
                if constexpr (LDIM == 3) Z[tid] = g[d][2] * s;
            }
            __syncthreads();
            if (live) t[d * t_stride + p] = transposed_line_sums<LDIM, NX>(q, X, Y, Z);
        }
    }
}

// ------------------------------------------------------------------------------------------
// The pointwise third of a CG iteration on the pressure mesh.  Every workgroup forms the scalars from the
// partials (cg_scalar):  mu = closed ? sum Ep / n : 0,  alpha = r.r / (p.Ep - mu sum p)  (0 when that is 0),
// then per point, without contraction,
//   x <- x + alpha p      r <- r - alpha (Ep - mu)
// and writes its partial of the new r.r into its slot.  init: x <- 0, r <- Ep - mu (the right-hand side with
// its mean removed), no p.  Thread-to-point map and block sums are fixed: the same bits run to run.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_pressure_cg_update(int64_t n, double* __restrict__ x,
                                                                 double* __restrict__ r, const double* __restrict__ p,
                                                                 const double* __restrict__ Ep,
                                                                 const double* __restrict__ red, int Br,
                                                                 const double* __restrict__ rr_old, int Bo, double inv_n,
                                                                 int closed, int init, double* __restrict__ rr_out) {
#pragma clang fp contract(off)
    __shared__ double sc[8];
    const double s_e = closed ? cg_scalar(red + Br, Br, sc) : 0.0;
    const double mu = s_e * inv_n;
    double alpha = 0.0;
    if (!init) {
        const double p_e = cg_scalar(red, Br, sc + 1), s_p = cg_scalar(red + 2 * (int64_t)Br, Br, sc + 2);
        const double rr = cg_scalar(rr_old, Bo, sc + 3);
        const double den = p_e - mu * s_p;
        alpha = den != 0.0 ? rr / den : 0.0;
    }
    double s = 0.0;
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) {
        double rv;
        if (init) {
            x[i] = 0.0;
            rv = Ep[i] - mu;
        } else {
            x[i] = x[i] + alpha * p[i];
            rv = r[i] - alpha * (Ep[i] - mu);
        }
        r[i] = rv;
        s += rv * rv;
    }
    s = block_sum(s, sc + 4);
    if (threadIdx.x == 0) rr_out[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// The two-system forms: the CG of two right-hand sides on one mesh (the re and the im half of a pair vector)
// in one launch each.  The systems share the coordinates, the factors, D, I and w^: those are staged and formed
// once per element group and the tiles then serve system 0, then system 1, so the LDS is the single-system
// kernel's.  Per system the arithmetic, its order, the thread-to-point map, the grid and the slot of every
// workgroup are those of the single-system kernel: the same bits.  active: bit s = system s; an inactive system
// is neither read nor written.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_pressure_div2(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ Ig, const double* __restrict__ gwg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm, const double* u0,
    const double* u1, int64_t u_stride, const double* __restrict__ mult, double* out0, double* out1, const double* pv0,
    const double* pv1, double* __restrict__ partials, int active) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int M = NX - 2;
    constexpr int ppts = pressure_pts<LDIM, NX>();
    const int nt = epb * pts;
    const Head<NX> h(lds, Dg, Ig, gwg);
    const double* I = h.I;
    double* X = h.tiles;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    const int tid = threadIdx.x;
    const TilePoint<LDIM, NX> q(h.D, tid, nt);
    const int le = tid / pts, rr = tid - le * pts;
    const int eb = le * pts;
    const bool intile = tid < nt;
    const double* const us[2] = {u0, u1};
    double* const outs[2] = {out0, out1};
    const double* const pvs[2] = {pv0, pv1};
    double s_pe[2] = {0.0, 0.0}, s_e[2] = {0.0, 0.0}, s_p[2] = {0.0, 0.0};
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = intile && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and the head is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
        }
        __syncthreads();
        double g[3][3], jac;   // dead lanes compute garbage they never store
        geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
        const double m = live && mult ? mult[p] : 1.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!(active >> s & 1)) continue;   // (uniform over the grid)
            __syncthreads();   // every lane has formed its factors, the system before is interpolated: the tiles are free
            if (live) {
                double* tiles[3] = {X, Y, Z};
#pragma unroll
                for (int d = 0; d < LDIM; ++d) {
                    const double v = us[s][d * u_stride + p];
                    tiles[d][tid] = mult ? m * v : v;
                }
            }
            __syncthreads();
            double dv = 0.0;
            {
                const double* tiles[3] = {X, Y, Z};
#pragma unroll
                for (int d = 0; d < LDIM; ++d) {
                    double ur, us_, ut;
                    line_sums<LDIM, NX>(q, tiles[d], ur, us_, ut);
                    double t = g[d][0] * ur + g[d][1] * us_;
                    if constexpr (LDIM == 3) t = t + g[d][2] * ut;
                    dv = d == 0 ? t : dv + t;
                }
            }
            __syncthreads();       // the velocity tiles are read
            if (intile) X[tid] = dv;
            __syncthreads();
            // along r: X(i, j, k) -> Y(a, j, k), a < M
            constexpr int n1 = LDIM == 3 ? M * NX * NX : M * NX;
            if (intile && rr < n1) {
                const int a = rr % M, row = rr / M;          // row = j + NX k
                const double* src = X + eb + row * NX;
                double acc = I[a * NX] * src[0];
#pragma unroll 2
                for (int mm = 1; mm < NX; ++mm) acc = acc + I[a * NX + mm] * src[mm];
                Y[eb + rr] = acc;
            }
            __syncthreads();
            // along s: Y(a, j, k) -> (a, b, k)
            constexpr int n2 = LDIM == 3 ? M * M * NX : M * M;
            double val = 0.0;
            if (intile && rr < n2) {
                const int a = rr % M, b = (rr / M) % M, k = rr / (M * M);
                const double* src = Y + eb + a + M * NX * k;
                double acc = I[b * NX] * src[0];
#pragma unroll 2
                for (int mm = 1; mm < NX; ++mm) acc = acc + I[b * NX + mm] * src[M * mm];
                if constexpr (LDIM == 3) X[eb + rr] = acc;
                val = acc;
            }
            if constexpr (LDIM == 3) {
                __syncthreads();
                // along t: X(a, b, k) -> (a, b, c)
                if (intile && rr < ppts) {
                    const int c = rr / (M * M), ab = rr - c * M * M;
                    const double* src = X + eb + ab;
                    double acc = I[c * NX] * src[0];
#pragma unroll 2
                    for (int mm = 1; mm < NX; ++mm) acc = acc + I[c * NX + mm] * src[M * M * mm];
                    val = acc;
                }
            }
            if (live && rr < ppts) {
                const int a = rr % M, b = (rr / M) % M, c = LDIM == 3 ? rr / (M * M) : 0;
                const double wab = h.gw[a] * h.gw[b];
                const double wq = LDIM == 3 ? wab * h.gw[c] : wab;
                const double o = wq * val;
                const int64_t pp = (e0 + le) * ppts + rr;
                outs[s][pp] = o;
                if (partials) {
                    const double pe = pvs[s][pp];
                    s_pe[s] += pe * o;
                    s_e[s] += o;
                    s_p[s] += pe;
                }
            }
        }
    }
    if (partials) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!(active >> s & 1)) continue;
            block_sum3(s_pe[s], s_e[s], s_p[s], h.red);
            if (tid == 0) {
                double* part = partials + (int64_t)s * 3 * kPB;
                part[blockIdx.x] = s_pe[s];
                part[kPB + blockIdx.x] = s_e[s];
                part[2 * kPB + blockIdx.x] = s_p[s];
            }
        }
    }
}

template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_pressure_gradt2(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ Ig, const double* __restrict__ gwg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm, double* p0, double* p1,
    const double* res0, const double* res1, const double* __restrict__ rr_new, const double* __restrict__ rr_old, int B,
    int first, double* t0, double* t1, int64_t t_stride, int active, const double* __restrict__ zsum, double inv_n) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int M = NX - 2;
    constexpr int ppts = pressure_pts<LDIM, NX>();
    const int nt = epb * pts;
    const Head<NX> h(lds, Dg, Ig, gwg);
    const double* I = h.I;
    double* X = h.tiles;
    double* Y = X + nt;
    double* Z = Y + nt;                      // 3-D only
    double* A = LDIM == 3 ? Z + nt : Z;
    double* Bt = A + nt;
    const int tid = threadIdx.x;
    double* const pins[2] = {p0, p1};
    const double* const ress[2] = {res0, res1};
    double* const ts[2] = {t0, t1};
    const bool with_res = res0 || res1;
    double beta[2] = {0.0, 0.0};
    if (with_res && !first) {   // (uniform over the grid)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!(active >> s & 1)) continue;
            const double num = cg_scalar(rr_new + (int64_t)s * B, B, h.red + 2 * s);
            const double den = cg_scalar(rr_old + (int64_t)s * B, B, h.red + 2 * s + 1);
            beta[s] = den != 0.0 ? num / den : 0.0;
        }
    }
    double zeta[2] = {0.0, 0.0};   // the preconditioned iteration: the mean of M r_s (uniform over the grid)
    if (with_res && zsum) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!(active >> s & 1)) continue;
            zeta[s] = cg_scalar(zsum + (int64_t)s * B, B, h.red + 4 + s) * inv_n;
        }
    }
    const TilePoint<LDIM, NX> q(h.D, tid, nt);
    const int le = tid / pts, rr = tid - le * pts;
    const int eb = le * pts;
    const bool intile = tid < nt;
    const int pi = q.i;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const int64_t p = e0 * pts + tid;
        const bool live = intile && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and the head is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
        }
        __syncthreads();
        double g[3][3], jac;   // dead lanes compute garbage they never store
        geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!(active >> s & 1)) continue;   // (uniform over the grid)
            // (the interpolation tiles were last read before the barriers of the flux loop of the system before)
            if (live && rr < ppts) {
                const int a = rr % M, b = (rr / M) % M, c = LDIM == 3 ? rr / (M * M) : 0;
                const double wab = h.gw[a] * h.gw[b];
                const double wq = LDIM == 3 ? wab * h.gw[c] : wab;
                const int64_t pp = (e0 + le) * ppts + rr;
                double v;
                if (with_res) {
                    double rv = ress[s][pp];
                    if (zsum) rv = rv - zeta[s];
                    v = first ? rv : rv + beta[s] * pins[s][pp];
                    pins[s][pp] = v;
                } else {
                    v = pins[s][pp];
                }
                A[eb + rr] = wq * v;
            }
            __syncthreads();   // w^ p is staged; every lane has formed its factors, the fluxes of the system before are read
            double* S1 = A;        // the tile the transposed s pass reads
            double* S2 = Bt;       // ... and writes
            if constexpr (LDIM == 3) {
                // along t, transposed: A(a, b, c) -> Bt(a, b, k)
                if (intile && rr < M * M * NX) {
                    const int k = rr / (M * M), ab = rr - k * M * M;
                    const double* src = A + eb + ab;
                    double acc = I[k] * src[0];
#pragma unroll 2
                    for (int c = 1; c < M; ++c) acc = acc + I[c * NX + k] * src[M * M * c];
                    Bt[eb + rr] = acc;
                }
                __syncthreads();
                S1 = Bt;
                S2 = A;
            }
            // along s, transposed: S1(a, b, k) -> S2(a, j, k)
            constexpr int n2 = LDIM == 3 ? M * NX * NX : M * NX;
            if (intile && rr < n2) {
                const int a = rr % M, j = (rr / M) % NX, k = rr / (M * NX);
                const double* src = S1 + eb + a + M * M * k;
                double acc = I[j] * src[0];
#pragma unroll 2
                for (int b = 1; b < M; ++b) acc = acc + I[b * NX + j] * src[M * b];
                S2[eb + rr] = acc;
            }
            __syncthreads();
            // along r, transposed: S2(a, j, k) -> the GLL point (i, j, k)
            double sv = 0.0;
            if (intile) {
                const double* src = S2 + eb + M * (rr / NX);
                sv = I[pi] * src[0];
#pragma unroll 2
                for (int a = 1; a < M; ++a) sv = sv + I[a * NX + pi] * src[a];
            }
#pragma unroll
            for (int d = 0; d < LDIM; ++d) {
                if (d > 0) __syncthreads();   // the previous direction's fluxes are read
                if (intile) {
                    X[tid] = g[d][0] * sv;
                    Y[tid] = g[d][1] * sv;
                    if constexpr (LDIM == 3) Z[tid] = g[d][2] * sv;
                }
                __syncthreads();
                if (live) ts[s][d * t_stride + p] = transposed_line_sums<LDIM, NX>(q, X, Y, Z);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_pressure_cg_update2(
    int64_t n, double* x0, double* x1, double* r0, double* r1, const double* p0, const double* p1, const double* Ep0,
    const double* Ep1, const double* __restrict__ red, int Br, const double* __restrict__ rr_old, int Bo, double inv_n,
    int closed, int init, double* __restrict__ rr_out, int active) {
#pragma clang fp contract(off)
    __shared__ double sc2[16];
    double* const xs[2] = {x0, x1};
    double* const rs[2] = {r0, r1};
    const double* const ps[2] = {p0, p1};
    const double* const Eps[2] = {Ep0, Ep1};
    const int64_t step = (int64_t)gridDim.x * kThreads;
#pragma unroll
    for (int sy = 0; sy < 2; ++sy) {
        if (!(active >> sy & 1)) continue;   // (uniform over the grid)
        double* sc = sc2 + 8 * sy;
        const double* rd = red + (int64_t)sy * 3 * Br;
        double* x = xs[sy];
        double* r = rs[sy];
        const double* p = ps[sy];
        const double* Ep = Eps[sy];
        const double s_e = closed ? cg_scalar(rd + Br, Br, sc) : 0.0;
        const double mu = s_e * inv_n;
        double alpha = 0.0;
        if (!init) {
            const double p_e = cg_scalar(rd, Br, sc + 1), s_p = cg_scalar(rd + 2 * (int64_t)Br, Br, sc + 2);
            const double rr = cg_scalar(rr_old + (int64_t)sy * Bo, Bo, sc + 3);
            const double den = p_e - mu * s_p;
            alpha = den != 0.0 ? rr / den : 0.0;
        }
        double s = 0.0;
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) {
            double rv;
            if (init) {
                x[i] = 0.0;
                rv = Ep[i] - mu;
            } else {
                x[i] = x[i] + alpha * p[i];
                rv = r[i] - alpha * (Ep[i] - mu);
            }
            r[i] = rv;
            s += rv * rv;
        }
        s = block_sum(s, sc + 4);
        if (threadIdx.x == 0) rr_out[(int64_t)sy * kPB + blockIdx.x] = s;
    }
}

template <int LDIM, int NX>
void launch_div(int64_t nel, const double* D, const double* I, const double* gw, const double* xm, const double* ym,
                const double* zm, const double* u, int64_t u_stride, const double* mult, double* out, const double* pv,
                double* partials, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)head_doubles<NX>() + (size_t)LDIM * epb * pts);
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, kPB);
    hipLaunchKernelGGL((k_pressure_div<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D, I, gw,
                       xm, ym, zm, u, u_stride, mult, out, pv, partials);
}

template <int LDIM, int NX>
void launch_gradt(int64_t nel, const double* D, const double* I, const double* gw, const double* xm, const double* ym,
                  const double* zm, double* p, const double* res, const double* rr_new, const double* rr_old, int B,
                  int first, double* t, int64_t t_stride, const double* zsum, double inv_n, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)head_doubles<NX>() + (size_t)(LDIM + 2) * epb * pts);
    static_assert(sizeof(double) * (head_doubles<10>() + 5 * 1000) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 4 * kPB);
    hipLaunchKernelGGL((k_pressure_gradt<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D, I,
                       gw, xm, ym, zm, p, res, rr_new, rr_old, B, first, t, t_stride, zsum, inv_n);
}

// The two-system launches: the grids, the block sizes and the LDS of launch_div and launch_gradt.
template <int LDIM, int NX>
void launch_div2(int64_t nel, const double* D, const double* I, const double* gw, const double* xm, const double* ym,
                 const double* zm, const double* u0, const double* u1, int64_t u_stride, const double* mult, double* out0,
                 double* out1, const double* pv0, const double* pv1, double* partials, int active, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)head_doubles<NX>() + (size_t)LDIM * epb * pts);
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, kPB);
    hipLaunchKernelGGL((k_pressure_div2<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D, I,
                       gw, xm, ym, zm, u0, u1, u_stride, mult, out0, out1, pv0, pv1, partials, active);
}

template <int LDIM, int NX>
void launch_gradt2(int64_t nel, const double* D, const double* I, const double* gw, const double* xm, const double* ym,
                   const double* zm, double* p0, double* p1, const double* res0, const double* res1, const double* rr_new,
                   const double* rr_old, int B, int first, double* t0, double* t1, int64_t t_stride, int active,
                   const double* zsum, double inv_n, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    const size_t lds = sizeof(double) * ((size_t)head_doubles<NX>() + (size_t)(LDIM + 2) * epb * pts);
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 4 * kPB);
    hipLaunchKernelGGL((k_pressure_gradt2<LDIM, NX>), dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, D, I,
                       gw, xm, ym, zm, p0, p1, res0, res1, rr_new, rr_old, B, first, t0, t1, t_stride, active, zsum, inv_n);
}

// ------------------------------------------------------------------------------------------
// The fast-diagonalisation preconditioner: z_e = M_e r_e on the pressure mesh,
//   M_e = (S x .. x S) diag( 1 / sum_d c[e][d] lambda_{i_d} ) (S^T x .. x S^T),     i_1 along r
// with S (M x M, row-major; S^T B^ S = I) and lambda the generalised eigenpairs of the 1-D reference problem and
// c[e][d] the ldim scalars of element e (pressure.py builds all three).  It touches the pressure mesh only: whole
// elements per workgroup (256 / M^ldim of them when that is more than one), one pressure point per thread.
// S^T along r, s[, t] by sum factorisation, ping-pong between two LDS tiles, the scale in registers, S back along
// t[, s], r; the last pass stays in registers.  LDS: S twice (as it is and transposed, so that the coefficient a
// lane reads is always indexed by the lane's own fastest-varying index: consecutive addresses), lambda, and the two
// tiles with the r rows padded to an odd length MP = M | 1: the r passes read rows (lanes of one row share an
// address, rows lie MP doubles apart: with 8-byte reads banked per 32-lane half no two rows of a half meet on a
// bank for M <= 8), the s and t passes read at strides MP and MP M with the lane index a consecutive.
// NSYS = 2 serves two systems with one staging of S and one set of denominators; per system the arithmetic, its
// order, the thread-to-point map, the grid and the slots are those of NSYS = 1: the same bits.  With partials
// given workgroup b writes its share of r_s.z_s to partials[s kPB + b] and of sum z_s to
// partials[(NSYS + s) kPB + b].  No atomics, no contraction; element-local.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
constexpr int pc_epb() { return pressure_pts<LDIM, NX>() >= 256 ? 1 : 256 / pressure_pts<LDIM, NX>(); }
template <int LDIM, int NX>
constexpr int pc_threads() { return (pc_epb<LDIM, NX>() * pressure_pts<LDIM, NX>() + 63) / 64 * 64; }
template <int LDIM, int NX>
constexpr int pc_tile() { return ((NX - 2) | 1) * (LDIM == 3 ? (NX - 2) * (NX - 2) : (NX - 2)); }
template <int LDIM, int NX>
constexpr int pc_lds_doubles() {
    return 2 * (NX - 2) * (NX - 2) + (NX - 2) + (NX & 1) + 3 * kMaxWaves + 2 * pc_epb<LDIM, NX>() * pc_tile<LDIM, NX>();
}

template <int LDIM, int NX, int NSYS>
__global__ __launch_bounds__((pc_threads<LDIM, NX>())) void k_pressure_precond(
    int64_t nel, const double* __restrict__ Sg, const double* __restrict__ lamg, const double* __restrict__ cg,
    const double* r0, const double* r1, double* z0, double* z1, double* __restrict__ partials, int active) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int M = NX - 2;
    constexpr int MP = M | 1;
    constexpr int ppts = pressure_pts<LDIM, NX>();
    constexpr int TP = pc_tile<LDIM, NX>();
    constexpr int epb = pc_epb<LDIM, NX>();
    double* Sf = lds;                 // Sf[k M + a] = S[k][a]: out_a = sum_k S[k][a] v_k   (S^T v)
    double* Sb = Sf + M * M;          // Sb[k M + a] = S[a][k]: out_a = sum_k S[a][k] v_k   (S v)
    double* lam = Sb + M * M;
    double* red = lam + M + (NX & 1);
    double* T0 = red + 3 * kMaxWaves;
    double* T1 = T0 + epb * TP;
    const int tid = threadIdx.x;
    for (int t = tid; t < M * M; t += blockDim.x) {
        Sf[t] = Sg[t];
        Sb[t] = Sg[(t % M) * M + t / M];
    }
    for (int t = tid; t < M; t += blockDim.x) lam[t] = lamg[t];
    const int le = tid / ppts, q = tid - le * ppts;
    const int a = q % M, b = (q / M) % M, c = LDIM == 3 ? q / (M * M) : 0;
    const bool intile = le < epb;
    const int base = le * TP;
    const int own = base + a + MP * (b + M * c);
    const double* const rs[2] = {r0, r1};
    double* const zs[2] = {z0, z1};
    double s_rz[NSYS], s_z[NSYS];
#pragma unroll
    for (int s = 0; s < NSYS; ++s) s_rz[s] = s_z[s] = 0.0;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        const bool live = intile && e0 + le < nel;
        const int64_t pp = (e0 + le) * ppts + q;
        __syncthreads();   // S and lambda are staged (first pass); the last pass of the group before has read T1
        double inv = 0.0;  // lanes without an element carry zeros through the passes
        if (live) {
            const double* ce = cg + (e0 + le) * LDIM;
            double den = ce[0] * lam[a] + ce[1] * lam[b];
            if constexpr (LDIM == 3) den = den + ce[2] * lam[c];
            inv = 1.0 / den;
        }
#pragma unroll
        for (int s = 0; s < NSYS; ++s) {
            if (!(active >> s & 1)) continue;   // (uniform over the grid)
            // (every pass below ends in a barrier before the tile it read is written again: T0 is free here)
            const double rv = live ? rs[s][pp] : 0.0;
            double v = 0.0;
            if (intile) T0[own] = rv;
            __syncthreads();
            if (intile) {      // S^T along r: T0(k, b, c) -> T1(a, b, c)
                const double* src = T0 + own - a;
                v = Sf[a] * src[0];
#pragma unroll
                for (int k = 1; k < M; ++k) v = v + Sf[k * M + a] * src[k];
                T1[own] = v;
            }
            __syncthreads();
            if (intile) {      // S^T along s: T1(a, k, c) -> (a, b, c)
                const double* src = T1 + base + a + MP * M * c;
                v = Sf[b] * src[0];
#pragma unroll
                for (int k = 1; k < M; ++k) v = v + Sf[k * M + b] * src[MP * k];
            }
            if constexpr (LDIM == 3) {
                if (intile) T0[own] = v;
                __syncthreads();
                if (intile) {  // S^T along t: T0(a, b, k) -> (a, b, c)
                    const double* src = T0 + base + a + MP * b;
                    v = Sf[c] * src[0];
#pragma unroll
                    for (int k = 1; k < M; ++k) v = v + Sf[k * M + c] * src[MP * M * k];
                }
                v = v * inv;
                if (intile) T1[own] = v;
                __syncthreads();
                if (intile) {  // S along t: T1(a, b, k) -> T0(a, b, c)
                    const double* src = T1 + base + a + MP * b;
                    v = Sb[c] * src[0];
#pragma unroll
                    for (int k = 1; k < M; ++k) v = v + Sb[k * M + c] * src[MP * M * k];
                }
            } else {
                v = v * inv;
            }
            if (intile) T0[own] = v;
            __syncthreads();
            if (intile) {      // S along s: T0(a, k, c) -> T1(a, b, c)
                const double* src = T0 + base + a + MP * M * c;
                v = Sb[b] * src[0];
#pragma unroll
                for (int k = 1; k < M; ++k) v = v + Sb[k * M + b] * src[MP * k];
                T1[own] = v;
            }
            __syncthreads();
            if (intile) {      // S along r: T1(k, b, c) -> the point (a, b, c)
                const double* src = T1 + own - a;
                v = Sb[a] * src[0];
#pragma unroll
                for (int k = 1; k < M; ++k) v = v + Sb[k * M + a] * src[k];
            }
            if (live) {
                zs[s][pp] = v;
                s_rz[s] += rv * v;
                s_z[s] += v;
            }
        }
    }
    if (partials) {
#pragma unroll
        for (int s = 0; s < NSYS; ++s) {
            if (!(active >> s & 1)) continue;
            double unused = 0.0;
            block_sum3(s_rz[s], s_z[s], unused, red);
            if (tid == 0) {
                partials[(int64_t)s * kPB + blockIdx.x] = s_rz[s];
                partials[(int64_t)(NSYS + s) * kPB + blockIdx.x] = s_z[s];
            }
        }
    }
}

template <int LDIM, int NX, int NSYS>
void launch_precond(int64_t nel, const double* S_, const double* lam, const double* c, const double* r0, const double* r1,
                    double* z0, double* z1, double* partials, int active, hipStream_t st) {
    constexpr int epb = pc_epb<LDIM, NX>();
    static_assert(pc_threads<LDIM, NX>() <= 64 * kMaxWaves, "block_sum3 holds kMaxWaves waves");
    const size_t lds = sizeof(double) * (size_t)pc_lds_doubles<LDIM, NX>();
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, kPB);
    hipLaunchKernelGGL((k_pressure_precond<LDIM, NX, NSYS>), dim3(grid), dim3(pc_threads<LDIM, NX>()), lds, st, nel, S_, lam,
                       c, r0, r1, z0, z1, partials, active);
}

// The spans a two-system entry writes and reads (NULL operands are left out): no written span may meet another
// written span or a read one.  In a pair vector the halves interleave, so strided fields enter segment by segment.
struct Spans {
    struct One {
        const double* p;
        int64_t n;
        const char* name;
    };
    One out[10], in[14];
    int n_out = 0, n_in = 0;
    void add(One* list, int& cnt, const double* p, int64_t n, const char* name, int nfld = 1, int64_t stride = 0) {
        for (int f = 0; p && f < nfld; ++f) list[cnt++] = One{p + (int64_t)f * stride, n, name};
    }
    void writes(const double* p, int64_t n, const char* name, int nfld = 1, int64_t stride = 0) {
        add(out, n_out, p, n, name, nfld, stride);
    }
    void reads(const double* p, int64_t n, const char* name, int nfld = 1, int64_t stride = 0) {
        add(in, n_in, p, n, name, nfld, stride);
    }
    int check(const char* who) const {
        auto meet = [](const One& a, const One& b) { return a.p < b.p + b.n && b.p < a.p + a.n; };
        for (int i = 0; i < n_out; ++i) {
            for (int j = i + 1; j < n_out; ++j)
                if (meet(out[i], out[j]))
                    return fail(NKV_EINVAL, "%s: %s overlaps %s", who, out[i].name, out[j].name);
            for (int j = 0; j < n_in; ++j)
                if (meet(out[i], in[j])) return fail(NKV_EINVAL, "%s: %s overlaps %s", who, out[i].name, in[j].name);
        }
        return NKV_OK;
    }
};

int check_active(const char* who, int active) {
    if (active < 1 || active > 3) return fail(NKV_EINVAL, "%s: active=%d outside 1..3 (bit s = system s)", who, active);
    return NKV_OK;
}

int check_pressure_args(const char* who, const nkv_layout* L, int lx1, int ldim, const double* zm) {
    if (lx1 < 3 && lx1 >= 0 && (ldim == 2 || ldim == 3))
        return fail(NKV_EINVAL, "%s: lx1=%d: the pressure mesh has lx1 - 2 points per direction, lx1 >= 3", who, lx1);
    return check_mesh_args(who, L, lx1, ldim, zm);
}

// One switch case per supported lx1 of the pressure kernels (lx2 = lx1 - 2 >= 1).
#define NKV_PR_CASES(CALL) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8) CALL(9) CALL(10)

}  // namespace

extern "C" {

int nkv_pressure_div(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                     const double* xm, const double* ym, const double* zm, const double* u, int64_t u_stride,
                     const double* mult, double* out, const double* pv, double* partials, void* stream) {
    static const char who[] = "pressure_div";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch (its partial slots stay as they are)
    CHECK(check_pressure_args(who, L, lx1, ldim, zm));
    if (u_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: stride u_stride=%lld below n_v=%lld", who, (long long)u_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(interp, who, "interp"));
    CHECK(need(gw, who, "gw"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(u, who, "u"));
    CHECK(need(out, who, "out"));
    if (!pv != !partials) return fail(NKV_EINVAL, "%s: pv and partials are both NULL or neither", who);
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    hipStream_t st = S(stream);
#define NKV_PR_DIV(NX)                                                                                        \
    case NX:                                                                                                  \
        if (ldim == 3) launch_div<3, NX>(nel, D, interp, gw, xm, ym, zm, u, u_stride, mult, out, pv, partials, st); \
        else launch_div<2, NX>(nel, D, interp, gw, xm, ym, zm, u, u_stride, mult, out, pv, partials, st);     \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_DIV) }
#undef NKV_PR_DIV
    NKV_LAUNCHED();
    return NKV_OK;
}

// nkv_pressure_gradt and nkv_pressure_pgradt: the second with zsum (the B partials of sum M r; NULL: no shift).
static int pressure_gradt_entry(const char* who, const nkv_layout* L, int lx1, int ldim, const double* D,
                                const double* interp, const double* gw, const double* xm, const double* ym,
                                const double* zm, double* p, const double* res, const double* rr_new,
                                const double* rr_old, int B, int first, double* t, int64_t t_stride, const double* zsum,
                                double inv_n, void* stream) {
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch
    CHECK(check_pressure_args(who, L, lx1, ldim, zm));
    if (t_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: stride t_stride=%lld below n_v=%lld", who, (long long)t_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(interp, who, "interp"));
    CHECK(need(gw, who, "gw"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(p, who, "p"));
    CHECK(need(t, who, "t"));
    if (res && !first) {
        CHECK(need(rr_new, who, "rr_new"));
        CHECK(need(rr_old, who, "rr_old"));
        if (B < 1 || B > kPB) return fail(NKV_EINVAL, "%s: B=%d outside 1..%d", who, B, kPB);
    }
    if (zsum) {
        CHECK(need(res, who, "res (zsum shifts res)"));
        if (B < 1 || B > kPB) return fail(NKV_EINVAL, "%s: B=%d outside 1..%d", who, B, kPB);
        if (!std::isfinite(inv_n)) return fail(NKV_EINVAL, "%s: inv_n=%g", who, inv_n);
    }
    if (res == p) return fail(NKV_EINVAL, "%s: res is p", who);
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    hipStream_t st = S(stream);
#define NKV_PR_GT(NX)                                                                                                 \
    case NX:                                                                                                          \
        if (ldim == 3)                                                                                                \
            launch_gradt<3, NX>(nel, D, interp, gw, xm, ym, zm, p, res, rr_new, rr_old, B, first, t, t_stride, zsum,  \
                                inv_n, st);                                                                           \
        else                                                                                                          \
            launch_gradt<2, NX>(nel, D, interp, gw, xm, ym, zm, p, res, rr_new, rr_old, B, first, t, t_stride, zsum,  \
                                inv_n, st);                                                                           \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_GT) }
#undef NKV_PR_GT
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pressure_gradt(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                       const double* xm, const double* ym, const double* zm, double* p, const double* res,
                       const double* rr_new, const double* rr_old, int B, int first, double* t, int64_t t_stride,
                       void* stream) {
    return pressure_gradt_entry("pressure_gradt", L, lx1, ldim, D, interp, gw, xm, ym, zm, p, res, rr_new, rr_old, B,
                                first, t, t_stride, nullptr, 0.0, stream);
}

int nkv_pressure_pgradt(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                        const double* xm, const double* ym, const double* zm, double* p, const double* res,
                        const double* rr_new, const double* rr_old, const double* zsum, int B, double inv_n, int first,
                        double* t, int64_t t_stride, void* stream) {
    return pressure_gradt_entry("pressure_pgradt", L, lx1, ldim, D, interp, gw, xm, ym, zm, p, res, rr_new, rr_old, B,
                                first, t, t_stride, zsum, inv_n, stream);
}

int nkv_pressure_cg_update(int64_t n, double* x, double* r, const double* p, const double* Ep, const double* red, int Br,
                           const double* rr_old, int Bo, double inv_n, int closed, int init, double* rr_out,
                           void* stream) {
    static const char who[] = "pressure_cg_update";
    if (n < 0) return fail(NKV_EINVAL, "%s: n=%lld", who, (long long)n);
    CHECK(need(rr_out, who, "rr_out"));
    if (n > 0) {
        CHECK(need(x, who, "x"));
        CHECK(need(r, who, "r"));
        CHECK(need(Ep, who, "Ep"));
    }
    if (!init) {
        CHECK(need(red, who, "red"));
        CHECK(need(rr_old, who, "rr_old"));
        if (n > 0) CHECK(need(p, who, "p"));
        if (Bo < 1 || Bo > kPB) return fail(NKV_EINVAL, "%s: Bo=%d outside 1..%d", who, Bo, kPB);
    }
    if (closed) CHECK(need(red, who, "red"));
    if ((closed || !init) && (Br < 1 || Br > kPB)) return fail(NKV_EINVAL, "%s: Br=%d outside 1..%d", who, Br, kPB);
    if (!std::isfinite(inv_n)) return fail(NKV_EINVAL, "%s: inv_n=%g", who, inv_n);
    // (an empty shard still launches one workgroup: it writes a zero partial)
    const int grid = grid_for(n, kPB);
    hipLaunchKernelGGL(k_pressure_cg_update, dim3(grid), dim3(kThreads), 0, S(stream), n, x, r, p, Ep, red, Br, rr_old, Bo,
                       inv_n, closed, init, rr_out);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pressure_div2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                      const double* xm, const double* ym, const double* zm, const double* u0, const double* u1,
                      int64_t u_stride, const double* mult, double* out0, double* out1, const double* pv0,
                      const double* pv1, double* partials, int active, void* stream) {
    static const char who[] = "pressure_div2";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch (its partial slots stay as they are)
    CHECK(check_pressure_args(who, L, lx1, ldim, zm));
    CHECK(check_active(who, active));
    if (u_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: stride u_stride=%lld below n_v=%lld", who, (long long)u_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(interp, who, "interp"));
    CHECK(need(gw, who, "gw"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    const int64_t npz = nel * (ldim == 3 ? (lx1 - 2) * (lx1 - 2) * (lx1 - 2) : (lx1 - 2) * (lx1 - 2));
    static const char* const un[2] = {"u0", "u1"};
    static const char* const on[2] = {"out0", "out1"};
    static const char* const pn[2] = {"pv0", "pv1"};
    const double* const us[2] = {u0, u1};
    double* const outs[2] = {out0, out1};
    const double* const pvs[2] = {pv0, pv1};
    Spans sp;
    sp.reads(mult, L->n_v, "mult");
    for (int s = 0; s < 2; ++s) {
        if (!(active >> s & 1)) continue;
        CHECK(need(us[s], who, un[s]));
        CHECK(need(outs[s], who, on[s]));
        if (!pvs[s] != !partials)
            return fail(NKV_EINVAL, "%s: %s and partials are both NULL or neither", who, pn[s]);
        sp.reads(us[s], L->n_v, un[s], ldim, u_stride);
        sp.reads(pvs[s], npz, pn[s]);
        sp.writes(outs[s], npz, on[s]);
        if (partials) sp.writes(partials + (int64_t)s * 3 * kPB, 3 * kPB, "partials");
    }
    CHECK(sp.check(who));
    hipStream_t st = S(stream);
#define NKV_PR_DIV2(NX)                                                                                          \
    case NX:                                                                                                     \
        if (ldim == 3)                                                                                           \
            launch_div2<3, NX>(nel, D, interp, gw, xm, ym, zm, u0, u1, u_stride, mult, out0, out1, pv0, pv1,     \
                               partials, active, st);                                                            \
        else                                                                                                     \
            launch_div2<2, NX>(nel, D, interp, gw, xm, ym, zm, u0, u1, u_stride, mult, out0, out1, pv0, pv1,     \
                               partials, active, st);                                                            \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_DIV2) }
#undef NKV_PR_DIV2
    NKV_LAUNCHED();
    return NKV_OK;
}

// nkv_pressure_gradt2 and nkv_pressure_pgradt2: the second with zsum (system s at zsum + s*B; NULL: no shift).
static int pressure_gradt2_entry(const char* who, const nkv_layout* L, int lx1, int ldim, const double* D,
                                 const double* interp, const double* gw, const double* xm, const double* ym,
                                 const double* zm, double* p0, double* p1, const double* res0, const double* res1,
                                 const double* rr_new, const double* rr_old, int B, int first, double* t0, double* t1,
                                 int64_t t_stride, int active, const double* zsum, double inv_n, void* stream) {
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch
    CHECK(check_pressure_args(who, L, lx1, ldim, zm));
    CHECK(check_active(who, active));
    if (t_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: stride t_stride=%lld below n_v=%lld", who, (long long)t_stride, (long long)L->n_v);
    CHECK(need(D, who, "D"));
    CHECK(need(interp, who, "interp"));
    CHECK(need(gw, who, "gw"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    const int64_t npz = nel * (ldim == 3 ? (lx1 - 2) * (lx1 - 2) * (lx1 - 2) : (lx1 - 2) * (lx1 - 2));
    static const char* const pn[2] = {"p0", "p1"};
    static const char* const rn[2] = {"res0", "res1"};
    static const char* const tn[2] = {"t0", "t1"};
    double* const ps[2] = {p0, p1};
    const double* const ress[2] = {res0, res1};
    double* const ts[2] = {t0, t1};
    const bool with_res = ress[active & 1 ? 0 : 1] != nullptr;   // decided by the first active system
    Spans sp;
    for (int s = 0; s < 2; ++s) {
        if (!(active >> s & 1)) continue;
        CHECK(need(ps[s], who, pn[s]));
        CHECK(need(ts[s], who, tn[s]));
        if ((ress[s] != nullptr) != with_res)
            return fail(NKV_EINVAL, "%s: res0 and res1 of the active systems are both NULL or neither", who);
        sp.writes(ts[s], L->n_v, tn[s], ldim, t_stride);
        if (with_res) {
            sp.writes(ps[s], npz, pn[s]);
            sp.reads(ress[s], npz, rn[s]);
        } else {
            sp.reads(ps[s], npz, pn[s]);
        }
    }
    if (with_res && !first) {
        CHECK(need(rr_new, who, "rr_new"));
        CHECK(need(rr_old, who, "rr_old"));
        if (B < 1 || B > kPB) return fail(NKV_EINVAL, "%s: B=%d outside 1..%d", who, B, kPB);
        sp.reads(rr_new, 2 * (int64_t)B, "rr_new");
        sp.reads(rr_old, 2 * (int64_t)B, "rr_old");
    }
    if (zsum) {
        if (!with_res) return fail(NKV_EINVAL, "%s: zsum shifts res0 / res1, which are NULL", who);
        if (B < 1 || B > kPB) return fail(NKV_EINVAL, "%s: B=%d outside 1..%d", who, B, kPB);
        if (!std::isfinite(inv_n)) return fail(NKV_EINVAL, "%s: inv_n=%g", who, inv_n);
        sp.reads(zsum, 2 * (int64_t)B, "zsum");
    }
    CHECK(sp.check(who));
    if (!(active & 1)) res0 = nullptr;   // the kernel takes the res path when either is given
    if (!(active & 2)) res1 = nullptr;
    hipStream_t st = S(stream);
#define NKV_PR_GT2(NX)                                                                                              \
    case NX:                                                                                                         \
        if (ldim == 3)                                                                                               \
            launch_gradt2<3, NX>(nel, D, interp, gw, xm, ym, zm, p0, p1, res0, res1, rr_new, rr_old, B, first, t0,   \
                                 t1, t_stride, active, zsum, inv_n, st);                                             \
        else                                                                                                         \
            launch_gradt2<2, NX>(nel, D, interp, gw, xm, ym, zm, p0, p1, res0, res1, rr_new, rr_old, B, first, t0,   \
                                 t1, t_stride, active, zsum, inv_n, st);                                             \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_GT2) }
#undef NKV_PR_GT2
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pressure_gradt2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                        const double* xm, const double* ym, const double* zm, double* p0, double* p1, const double* res0,
                        const double* res1, const double* rr_new, const double* rr_old, int B, int first, double* t0,
                        double* t1, int64_t t_stride, int active, void* stream) {
    return pressure_gradt2_entry("pressure_gradt2", L, lx1, ldim, D, interp, gw, xm, ym, zm, p0, p1, res0, res1, rr_new,
                                 rr_old, B, first, t0, t1, t_stride, active, nullptr, 0.0, stream);
}

int nkv_pressure_pgradt2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                         const double* xm, const double* ym, const double* zm, double* p0, double* p1, const double* res0,
                         const double* res1, const double* rr_new, const double* rr_old, const double* zsum, int B,
                         double inv_n, int first, double* t0, double* t1, int64_t t_stride, int active, void* stream) {
    return pressure_gradt2_entry("pressure_pgradt2", L, lx1, ldim, D, interp, gw, xm, ym, zm, p0, p1, res0, res1, rr_new,
                                 rr_old, B, first, t0, t1, t_stride, active, zsum, inv_n, stream);
}

int nkv_pressure_cg_update2(int64_t n, double* x0, double* x1, double* r0, double* r1, const double* p0, const double* p1,
                            const double* Ep0, const double* Ep1, const double* red, int Br, const double* rr_old, int Bo,
                            double inv_n, int closed, int init, double* rr_out, int active, void* stream) {
    static const char who[] = "pressure_cg_update2";
    if (n < 0) return fail(NKV_EINVAL, "%s: n=%lld", who, (long long)n);
    CHECK(check_active(who, active));
    CHECK(need(rr_out, who, "rr_out"));
    if (!init) {
        CHECK(need(red, who, "red"));
        CHECK(need(rr_old, who, "rr_old"));
        if (Bo < 1 || Bo > kPB) return fail(NKV_EINVAL, "%s: Bo=%d outside 1..%d", who, Bo, kPB);
    }
    if (closed) CHECK(need(red, who, "red"));
    if ((closed || !init) && (Br < 1 || Br > kPB)) return fail(NKV_EINVAL, "%s: Br=%d outside 1..%d", who, Br, kPB);
    if (!std::isfinite(inv_n)) return fail(NKV_EINVAL, "%s: inv_n=%g", who, inv_n);
    static const char* const xn[2] = {"x0", "x1"};
    static const char* const rn[2] = {"r0", "r1"};
    static const char* const pn[2] = {"p0", "p1"};
    static const char* const en[2] = {"Ep0", "Ep1"};
    double* const xs[2] = {x0, x1};
    double* const rs[2] = {r0, r1};
    const double* const ps[2] = {p0, p1};
    const double* const Eps[2] = {Ep0, Ep1};
    Spans sp;
    for (int s = 0; s < 2; ++s) {
        if (!(active >> s & 1)) continue;
        if (n > 0) {
            CHECK(need(xs[s], who, xn[s]));
            CHECK(need(rs[s], who, rn[s]));
            CHECK(need(Eps[s], who, en[s]));
            if (!init) CHECK(need(ps[s], who, pn[s]));
            sp.writes(xs[s], n, xn[s]);
            sp.writes(rs[s], n, rn[s]);
            sp.reads(Eps[s], n, en[s]);
            if (!init) sp.reads(ps[s], n, pn[s]);
        }
        sp.writes(rr_out + (int64_t)s * kPB, kPB, "rr_out");
        if (closed || !init) sp.reads(red + (int64_t)s * 3 * Br, 3 * (int64_t)Br, "red");
        if (!init) sp.reads(rr_old + (int64_t)s * Bo, Bo, "rr_old");
    }
    CHECK(sp.check(who));
    // (an empty shard still launches one workgroup: it writes a zero partial for every active system)
    const int grid = grid_for(n, kPB);
    hipLaunchKernelGGL(k_pressure_cg_update2, dim3(grid), dim3(kThreads), 0, S(stream), n, x0, x1, r0, r1, p0, p1, Ep0, Ep1,
                       red, Br, rr_old, Bo, inv_n, closed, init, rr_out, active);
    NKV_LAUNCHED();
    return NKV_OK;
}

static int check_precond_args(const char* who, int64_t nel, int lx1, int ldim, const double* S_, const double* lam,
                              const double* c) {
    if (nel < 0) return fail(NKV_EINVAL, "%s: nel=%lld", who, (long long)nel);
    if (ldim != 2 && ldim != 3) return fail(NKV_EINVAL, "%s: ldim=%d (2 or 3)", who, ldim);
    if (lx1 < 3 || lx1 > 10) return fail(NKV_EINVAL, "%s: lx1=%d outside 3..10", who, lx1);
    CHECK(need(S_, who, "S"));
    CHECK(need(lam, who, "lambda"));
    CHECK(need(c, who, "c"));
    return NKV_OK;
}

int nkv_pressure_precond(int64_t nel, int lx1, int ldim, const double* S_, const double* lam, const double* c,
                         const double* r, double* z, double* partials, void* stream) {
    static const char who[] = "pressure_precond";
    CHECK(check_precond_args(who, nel, lx1, ldim, S_, lam, c));
    if (nel == 0) return NKV_OK;   // an empty shard: nothing to touch (its partial slots stay as they are)
    CHECK(need(r, who, "r"));
    CHECK(need(z, who, "z"));
    const int m = lx1 - 2;
    const int64_t npz = nel * (ldim == 3 ? m * m * m : m * m);
    Spans sp;
    sp.reads(r, npz, "r");
    sp.writes(z, npz, "z");
    if (partials) sp.writes(partials, 2 * (int64_t)kPB, "partials");
    CHECK(sp.check(who));
    hipStream_t st = S(stream);
#define NKV_PR_PC(NX)                                                                                    \
    case NX:                                                                                             \
        if (ldim == 3) launch_precond<3, NX, 1>(nel, S_, lam, c, r, nullptr, z, nullptr, partials, 1, st); \
        else launch_precond<2, NX, 1>(nel, S_, lam, c, r, nullptr, z, nullptr, partials, 1, st);         \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_PC) }
#undef NKV_PR_PC
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pressure_precond2(int64_t nel, int lx1, int ldim, const double* S_, const double* lam, const double* c,
                          const double* r0, const double* r1, double* z0, double* z1, double* partials, int active,
                          void* stream) {
    static const char who[] = "pressure_precond2";
    CHECK(check_precond_args(who, nel, lx1, ldim, S_, lam, c));
    CHECK(check_active(who, active));
    if (nel == 0) return NKV_OK;   // an empty shard: nothing to touch (its partial slots stay as they are)
    const int m = lx1 - 2;
    const int64_t npz = nel * (ldim == 3 ? m * m * m : m * m);
    static const char* const rn[2] = {"r0", "r1"};
    static const char* const zn[2] = {"z0", "z1"};
    const double* const rs[2] = {r0, r1};
    double* const zs[2] = {z0, z1};
    Spans sp;
    for (int s = 0; s < 2; ++s) {
        if (!(active >> s & 1)) continue;
        CHECK(need(rs[s], who, rn[s]));
        CHECK(need(zs[s], who, zn[s]));
        sp.reads(rs[s], npz, rn[s]);
        sp.writes(zs[s], npz, zn[s]);
        if (partials) {
            sp.writes(partials + (int64_t)s * kPB, kPB, "partials");
            sp.writes(partials + (int64_t)(2 + s) * kPB, kPB, "partials");
        }
    }
    CHECK(sp.check(who));
    hipStream_t st = S(stream);
#define NKV_PR_PC2(NX)                                                                                   \
    case NX:                                                                                             \
        if (ldim == 3) launch_precond<3, NX, 2>(nel, S_, lam, c, r0, r1, z0, z1, partials, active, st);  \
        else launch_precond<2, NX, 2>(nel, S_, lam, c, r0, r1, z0, z1, partials, active, st);            \
        break;
    switch (lx1) { NKV_PR_CASES(NKV_PR_PC2) }
#undef NKV_PR_PC2
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_pressure_partials(void) { return kPB; }

}  // extern "C"
