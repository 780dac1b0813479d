// advdiff.hip — the spectral-element advection-diffusion of every dotted field by a frozen base flow U,
// the equation Nek5000 advances for a passive scalar (ifheat, t) and the model operator behind
// advdiff.AdvectionDiffusion (a LightKrylov abstract_linop whose matvec is a time integration,
// linear_operators.f90:39-103).  Weak form on the GLL mesh, per element and field u with diffusivity kappa:
//   forward:  r = -bm1 (U . grad u) + sum_a D_a^T [ sum_d (g[d][a] / jac) (-kappa bm1 d_d u) ]
//   adjoint:  r =                     sum_a D_a^T [ sum_d (g[d][a] / jac) (-kappa bm1 d_d u - bm1 U_d u) ]
// with g[d][a], jac the geometric factors of k_gradm1 (glmapm1 / xyzrst), d_d u the derivative exactly as
// k_gradm1 forms it, bm1 = jac w_i w_j [w_k] the mass matrix and D_a^T the transposed line sum along the
// reference direction a.  r is the LOCAL (unassembled) right-hand side: dssum and the inverse mass matrix
// follow as dsavg and the pointwise k_advdiff_stage.  No contraction; element-local, so it shards with the
// elements and any element sub-range gives the bits of the whole.
// Further down: the same right-hand side with the production term of a base state B of all fields
// (k_linconv_rhs: the linearisation of the viscous Burgers flow of burgers.py and its adjoint) and the
// classical RK4 stage of that flow (k_rk4_stage); its nonlinear right-hand side is k_advdiff_rhs with U = u.
// Last: the periodic orbits of that flow (orbit.py) — the nonlinear and the linearised right-hand side of a
// base state and a perturbation advanced side by side in one pass (k_burgers_tangent_rhs) and the RK4 stage
// under a harmonic forcing that writes the orbit, with the tangent's stage in the same launch (k_orbit_stage);
// and the linearised right-hand side of the re and the im half of a pair vector in one pass (k_linconv_crhs),
// the Horner pass of the coupled resolvent (resolvent.py); and the backward sweep of a checkpointed adjoint,
// the nonlinear right-hand side of a segment being recomputed and the adjoint one about a stored stage state in
// one pass (k_burgers_backward_rhs).
// The tiled kernels are assembled from shared blocks, and the next one should be too.  Device: TileFrame (the carve
// of the dynamic LDS, D staged, this thread's TilePoint and weight; begin_group stages an element group's
// coordinates and forms the factors, with the two barriers that takes), physical_gradient (line_sums and
// physical_derivative of one staged field), field_fluxes (the forward or the adjoint fluxes of one staged field
// into the tiles, through write_fluxes), presweep_field (one base field of the adjoint's first sweep) and
// transposed_line_sums (nkv_internal.h).  A kernel keeps its own field loop, its staging and the barriers between
// them: those are what differs.  Host: check_tiled_entry, spans_meet, dispatch_tile over lx1 x ldim and
// launch_tiled, which sizes the LDS from the number of field tiles.
#include <type_traits>

#include "nkv_internal.h"

namespace {

// ------------------------------------------------------------------------------------------
// The building blocks of the tiled kernels.
// ------------------------------------------------------------------------------------------

// The frame of a tiled kernel: the carve of the dynamic LDS (D, the LDIM coordinate tiles and up to two field
// tiles behind them: the launch sizes the LDS for the tiles the kernel uses), D staged, this thread's point and
// weight; and the head of every element group.
template <int LDIM, int NX>
struct TileFrame {
    static constexpr int pts = tile_pts<LDIM, NX>();
    const int tid, nt, le;
    double* const D;                         // D(i, m) at D[i*NX + m]
    double* const X;                         // coordinates, then the flux along r
    double* const Y;                         // ... along s
    double* const Z;                         // ... along t (3-D only)
    double* const U;                         // the first field tile (kernels with one or two)
    double* const Bt;                        // the second field tile (kernels with two)
    const TilePoint<LDIM, NX> q;
    double wt;                               // w_i w_j [w_k]

    __device__ __forceinline__ TileFrame(double* lds, int epb, const double* Dg, const double* wg)
        : tid(threadIdx.x), nt(epb * pts), le(tid / pts), D(lds), X(D + NX * NX), Y(X + nt), Z(Y + nt),
          U(LDIM == 3 ? Z + nt : Z), Bt(U + nt), q(D, tid, nt) {
        for (int t = tid; t < NX * NX; t += blockDim.x) D[t] = Dg[t];
        wt = q.weight(wg);
    }

    // The head of the element group at e0: stage its coordinates, form this point's factors.  Returns whether
    // this lane owns a point of the group (dead lanes compute garbage they never store); p: that point.
    __device__ __forceinline__ bool begin_group(int64_t e0, int64_t nel, const double* xm, const double* ym,
                                                const double* zm, int64_t& p, double (&g)[3][3], double& jac) const {
#pragma clang fp contract(off)
        p = e0 * pts + tid;
        const bool live = tid < nt && e0 + le < nel;
        __syncthreads();   // the previous group's reads are done (and D is staged on the first pass)
        if (live) {
            X[tid] = xm[p];
            Y[tid] = ym[p];
            if (LDIM == 3) Z[tid] = zm[p];
        }
        __syncthreads();
        geometric_factors_jac<LDIM, NX>(q, X, Y, Z, g, jac);
        return live;
    }
};

// The LDIM physical derivatives of one staged field at this point (line_sums, then physical_derivative).
template <int LDIM, int NX>
__device__ __forceinline__ void physical_gradient(const TilePoint<LDIM, NX>& q, const double* T,
                                                  const double (&g)[3][3], double jacmi, double (&dT)[LDIM]) {
#pragma clang fp contract(off)
    double tr, ts, tt;
    line_sums<LDIM, NX>(q, T, tr, ts, tt);
#pragma unroll
    for (int d = 0; d < LDIM; ++d) dT[d] = physical_derivative<LDIM>(g, jacmi, d, tr, ts, tt);
}

// The flux writer: F_a = sum_d (g[d][a] / jac) G_d into the three tiles.
template <int LDIM, int NX>
__device__ __forceinline__ void write_fluxes(const TileFrame<LDIM, NX>& t, const double (&g)[3][3], double jacmi,
                                             const double (&G)[LDIM]) {
#pragma clang fp contract(off)
    double* tiles[3] = {t.X, t.Y, t.Z};
#pragma unroll
    for (int a = 0; a < LDIM; ++a) {
        double F = g[0][a] * jacmi * G[0];
#pragma unroll
        for (int d = 1; d < LDIM; ++d) F = F + g[d][a] * jacmi * G[d];
        tiles[a][t.tid] = F;
    }
}

// The fluxes of the field staged in T into the three tiles, kb = -kappa bm1.
//   forward:  G_d = kb d_d u;  returns the advection sum_d Ub_d d_d u
//   adjoint:  G_d = kb d_d u - bm1 Ub_d u;  returns 0
template <bool ADJ, int LDIM, int NX>
__device__ __forceinline__ double field_fluxes(const TileFrame<LDIM, NX>& t, const double* T, const double (&g)[3][3],
                                               double jacmi, double bm, double kb, const double (&Ub)[LDIM]) {
#pragma clang fp contract(off)
    double du[LDIM], G[LDIM], adv = 0.0;
    physical_gradient<LDIM, NX>(t.q, T, g, jacmi, du);
#pragma unroll
    for (int d = 0; d < LDIM; ++d) {
        if constexpr (ADJ) {
            G[d] = kb * du[d] - bm * Ub[d] * T[t.tid];
        } else {
            G[d] = kb * du[d];
            adv = adv + Ub[d] * du[d];
        }
    }
    write_fluxes(t, g, jacmi, G);
    return adv;
}

// One base field of the adjoint pre-sweep, staged in T:  P_d <- [not first] P_d + u_f d_d B_f.
template <int LDIM, int NX>
__device__ __forceinline__ void presweep_field(const TilePoint<LDIM, NX>& q, const double* T, const double (&g)[3][3],
                                               double jacmi, double uf, bool first, double (&P)[LDIM]) {
#pragma clang fp contract(off)
    double db[LDIM];
    physical_gradient<LDIM, NX>(q, T, g, jacmi, db);
#pragma unroll
    for (int d = 0; d < LDIM; ++d) P[d] = first ? uf * db[d] : P[d] + uf * db[d];
}

// ------------------------------------------------------------------------------------------
// The fused right-hand side: the tile of k_gradm1 (whole elements per workgroup, one point per thread).
// The coordinates of a group of elements are staged in LDS and the factors formed once per group; then for
// every field: stage u, differentiate by line sums, write the LDIM reference-space fluxes
//   F_a = sum_d (g[d][a] / jac) G_d,   G_d = -kappa bm1 d_d u  [adjoint: - bm1 U_d u]
// over the coordinate tiles (their last reader, the factors, is a barrier behind), barrier, take the
// transposed line sums  sum_m D(m, i) F_r(m, j, k) + sum_m D(m, j) F_s(i, m, k) [+ sum_m D(m, k) F_t(i, j, m)]
// and store r once.  Neither the gradient nor the fluxes touch global memory.  LDS: lx1^2 + (LDIM + 1) nt
// doubles, 32,800 bytes at lx1 = 10 in 3-D.  Line sums unrolled by 2, as k_gradm1 measured.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX, bool ADJ>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_advdiff_rhs(
    int64_t nel, int epb, int nfld, const double* __restrict__ Dg, const double* __restrict__ wg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ ub, int64_t b_stride, const double* __restrict__ kappa, const double* __restrict__ u,
    int64_t u_stride, double* __restrict__ r, int64_t r_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);   // one field tile: U, the field being differentiated
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        const double jacmi = 1.0 / jac;
        const double bm = jac * t.wt;
        double Ub[LDIM];
#pragma unroll
        for (int d = 0; d < LDIM; ++d) Ub[d] = live ? ub[d * b_stride + p] : 0.0;
        for (int f = 0; f < nfld; ++f) {
            if (f > 0) __syncthreads();   // every lane is done reading the previous field and its fluxes
            if (live) t.U[t.tid] = u[f * u_stride + p];
            __syncthreads();              // (and every lane has formed its factors: the tiles are free)
            double adv = 0.0;
            if (live) adv = field_fluxes<ADJ>(t, t.U, g, jacmi, bm, -kappa[f] * bm, Ub);
            __syncthreads();
            if (live) {
                const double acc = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z);
                r[f * r_stride + p] = ADJ ? acc : acc - bm * adv;
            }
        }
    }
}

// bm1 = jac w_i w_j [w_k]: the factors' Jacobian times the GLL weights, the product the right-hand side forms.
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_advdiff_bm1(
    int64_t nel, int epb, const double* __restrict__ Dg, const double* __restrict__ wg, const double* __restrict__ xm,
    const double* __restrict__ ym, const double* __restrict__ zm, double* __restrict__ bm1) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);   // no field tile
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        if (live) bm1[p] = jac * t.wt;
    }
}

// ------------------------------------------------------------------------------------------
// One Horner stage of p(dt L) for all fields (grid.y = field):  w_f = v_f + c (m r_f),  m the pointwise
// inverse assembled mass matrix (mask / dsavg(bm1)) and r_f the averaged right-hand side.  v = NULL stands
// for zero, which makes the same kernel the two pointwise halves of the projector: bm1 x before the
// average, minv times the average after it (c = 1).  w may be v (pointwise).  On request field 0's blocks
// also zero the pressure rows and the time slot of w, as k_op_rot2 zeroes y[time_off].  VEC: two points
// per thread by 16-byte accesses; the odd last point goes to one thread.  No contraction, so both forms
// give the same bits.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_advdiff_stage(int64_t n, const double* v, int64_t v_stride,
                                                            const double* __restrict__ m, const double* r,
                                                            int64_t r_stride, double c, double* w, int64_t w_stride,
                                                            double* zero_p, int64_t n_p, double* zero_t) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const double* vf = v ? v + f * v_stride : nullptr;
    const double* rf = r + f * r_stride;
    double* wf = w + f * w_stride;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    auto point = [&](int64_t p) {
        const double t = c * (m[p] * rf[p]);
        wf[p] = vf ? vf[p] + t : t;
    };
    if constexpr (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = t0; i < pairs; i += step) {
            const int64_t p = 2 * i;
            const double2 mm = ld2(m + p), rr = ld2(rf + p);
            double2 o = make_double2(c * (mm.x * rr.x), c * (mm.y * rr.y));
            if (vf) {
                const double2 vv = ld2(vf + p);
                o = make_double2(vv.x + o.x, vv.y + o.y);
            }
            st2(wf + p, o);
        }
        if ((n & 1) && t0 == 0) point(n - 1);
    } else {
        for (int64_t p = t0; p < n; p += step) point(p);
    }
    if (f == 0 && zero_p) {
        for (int64_t p = t0; p < n_p; p += step) zero_p[p] = 0.0;
        if (t0 == 0) *zero_t = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// One Horner stage of p(dt G), G = L - i omega on complex fields kept as re / im halves, with a constant
// forcing inside (the rotating-frame resolvent of resolvent.py; linear_operators.f90:348-431 integrates the
// real state under cos / sin forcing instead).  Per point, in this order and without contraction:
//   g_re = (m r_re + omega s_im) [+ f_re]      g_im = (m r_im - omega s_re) [+ f_im]
//   w_re = v_re + c g_re                        w_im = v_im + c g_im
// r: the averaged right-hand sides of the two halves of the stage's source s; v = NULL stands for zero,
// f = NULL for no forcing.  One thread forms both halves of a point, so w may be v; w is never s, r, f or
// m (the entry refuses overlapping spans), which is what lets those carry __restrict__.  Nine reads and two
// writes per point and field in one launch; grid.y = field, the zeroing and VEC as in k_advdiff_stage.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_advdiff_cstage(
    int64_t n, const double* v_re, const double* v_im, int64_t v_stride, const double* __restrict__ m,
    const double* __restrict__ r_re, const double* __restrict__ r_im, int64_t r_stride,
    const double* __restrict__ s_re, const double* __restrict__ s_im, int64_t s_stride,
    const double* __restrict__ f_re, const double* __restrict__ f_im, int64_t f_stride, double omega, double c,
    double* w_re, double* w_im, int64_t w_stride, double* zero_p, int64_t n_p, double* zero_t) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const double* vr = v_re ? v_re + f * v_stride : nullptr;
    const double* vi = v_re ? v_im + f * v_stride : nullptr;
    const double* rr = r_re + f * r_stride;
    const double* ri = r_im + f * r_stride;
    const double* sr = s_re + f * s_stride;
    const double* si = s_im + f * s_stride;
    const double* fr = f_re ? f_re + f * f_stride : nullptr;
    const double* fi = f_re ? f_im + f * f_stride : nullptr;
    double* wr = w_re + f * w_stride;
    double* wi = w_im + f * w_stride;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    auto point = [&](int64_t p) {
        double gr = m[p] * rr[p] + omega * si[p];
        double gi = m[p] * ri[p] - omega * sr[p];
        if (fr) {
            gr = gr + fr[p];
            gi = gi + fi[p];
        }
        const double tr = c * gr, ti = c * gi;
        const double o_re = vr ? vr[p] + tr : tr, o_im = vr ? vi[p] + ti : ti;
        wr[p] = o_re;
        wi[p] = o_im;
    };
    if constexpr (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = t0; i < pairs; i += step) {
            const int64_t p = 2 * i;
            const double2 mm = ld2(m + p), a = ld2(rr + p), b = ld2(ri + p), x = ld2(sr + p), y = ld2(si + p);
            double2 gr = make_double2(mm.x * a.x + omega * y.x, mm.y * a.y + omega * y.y);
            double2 gi = make_double2(mm.x * b.x - omega * x.x, mm.y * b.y - omega * x.y);
            if (fr) {
                const double2 p_re = ld2(fr + p), p_im = ld2(fi + p);
                gr = make_double2(gr.x + p_re.x, gr.y + p_re.y);
                gi = make_double2(gi.x + p_im.x, gi.y + p_im.y);
            }
            double2 o_re = make_double2(c * gr.x, c * gr.y), o_im = make_double2(c * gi.x, c * gi.y);
            if (vr) {
                const double2 q_re = ld2(vr + p), q_im = ld2(vi + p);
                o_re = make_double2(q_re.x + o_re.x, q_re.y + o_re.y);
                o_im = make_double2(q_im.x + o_im.x, q_im.y + o_im.y);
            }
            st2(wr + p, o_re);
            st2(wi + p, o_im);
        }
        if ((n & 1) && t0 == 0) point(n - 1);
    } else {
        for (int64_t p = t0; p < n; p += step) point(p);
    }
    if (f == 0 && zero_p) {
        for (int64_t p = t0; p < n_p; p += step) zero_p[p] = 0.0;
        if (t0 == 0) *zero_t = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// The linearised convection about a base state B of n_wf fields (velocity first): k_advdiff_rhs with the
// advecting velocity B_0..B_{LDIM-1} plus the production term, for all fields in one launch.
//   forward:  r_f = r_advdiff,f(u; U = B_vel) - bm1 sum_{d<LDIM} u_d d_d B_f
//   adjoint:  r_f = r_advdiff,adj,f(u; U = B_vel) - [f < LDIM] bm1 sum_{f'<nfld} u_f' d_f B_f'
// d_d B_f as k_gradm1 forms it, from B_f staged in one more tile (Bt) and the same line sums: grad B never
// touches global memory.  The sums run in ascending index; the advection-diffusion part keeps the operand
// order of k_advdiff_rhs.
// Forward: B_f is staged next to u_f, no barrier more than k_advdiff_rhs.  Adjoint: velocity component d
// closes with sum_f' u_f' d_d B_f', so a first sweep over the base fields accumulates LDIM registers; it
// alternates between the two field tiles, one barrier per base field.  LDS: lx1^2 + (LDIM + 2) nt doubles,
// 40,800 bytes at lx1 = 10 in 3-D.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX, bool ADJ>
__global__ __launch_bounds__((tile_threads<LDIM, NX>())) void k_linconv_rhs(
    int64_t nel, int epb, int nfld, const double* __restrict__ Dg, const double* __restrict__ wg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ B, int64_t b_stride, const double* __restrict__ kappa, const double* __restrict__ u,
    int64_t u_stride, double* __restrict__ r, int64_t r_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    // two field tiles: U, the field being differentiated, and Bt, the base field being differentiated
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);
    const int tid = t.tid;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        const double jacmi = 1.0 / jac;
        const double bm = jac * t.wt;
        double Ub[LDIM];       // the advecting velocity B_d
        double P[LDIM];        // forward: the velocity perturbation u_d; adjoint: sum_f' u_f' d_d B_f'
#pragma unroll
        for (int d = 0; d < LDIM; ++d) {
            Ub[d] = live ? B[d * b_stride + p] : 0.0;
            P[d] = (!ADJ && live) ? u[d * u_stride + p] : 0.0;
        }
        if constexpr (ADJ) {
            for (int f = 0; f < nfld; ++f) {
                double* T = (f & 1) ? t.Bt : t.U;   // the tile written two fields ago: a barrier lies between
                if (live) T[tid] = B[f * b_stride + p];
                __syncthreads();
                if (live) presweep_field<LDIM, NX>(t.q, T, g, jacmi, u[f * u_stride + p], f == 0, P);
            }
        }
        for (int f = 0; f < nfld; ++f) {
            if (f > 0 || ADJ) __syncthreads();   // every lane is done reading the previous field and its fluxes
            if (live) {
                t.U[tid] = u[f * u_stride + p];
                if constexpr (!ADJ) t.Bt[tid] = B[f * b_stride + p];
            }
            __syncthreads();              // (and every lane has formed its factors: the tiles are free)
            double adv = 0.0, prod = 0.0;
            if (live) {
                if constexpr (!ADJ) {
                    double db[LDIM];
                    physical_gradient<LDIM, NX>(t.q, t.Bt, g, jacmi, db);
                    prod = P[0] * db[0];
#pragma unroll
                    for (int d = 1; d < LDIM; ++d) prod = prod + P[d] * db[d];
                } else {
#pragma unroll
                    for (int d = 0; d < LDIM; ++d)
                        if (f == d) prod = P[d];
                }
                adv = field_fluxes<ADJ>(t, t.U, g, jacmi, bm, -kappa[f] * bm, Ub);
            }
            __syncthreads();
            if (live) {
                const double acc = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z);
                if constexpr (ADJ)
                    r[f * r_stride + p] = f < LDIM ? acc - bm * prod : acc;
                else
                    r[f * r_stride + p] = (acc - bm * adv) - bm * prod;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// One stage of classical RK4 for all fields (grid.y = field).  Per point, in this order, no contraction:
//   k = m r [+ g]      w = v + a k      acc' = (first ? v : acc) + b k
// m: the pointwise inverse assembled mass matrix, r: the averaged right-hand side of the stage's state,
// g: a constant forcing.  v = NULL stands for zero, as in k_advdiff_stage.  w (the next stage's state) may be
// NULL; acc' goes to ao, which may be acc or v (one thread reads a point's operands before it writes them).
// The zeroing of the rest of a state vector and VEC as in k_advdiff_stage.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_rk4_stage(int64_t n, const double* v, int64_t v_stride,
                                                        const double* __restrict__ m, const double* __restrict__ r,
                                                        int64_t r_stride, const double* __restrict__ g,
                                                        int64_t g_stride, double a, double b, int first,
                                                        const double* acc, int64_t acc_stride, double* w,
                                                        int64_t w_stride, double* ao, int64_t ao_stride, double* zero_p,
                                                        int64_t n_p, double* zero_t) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const double* vf = v ? v + f * v_stride : nullptr;
    const double* rf = r + f * r_stride;
    const double* gf = g ? g + f * g_stride : nullptr;
    const double* af = first ? vf : acc + f * acc_stride;
    double* wf = w ? w + f * w_stride : nullptr;
    double* of = ao + f * ao_stride;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    auto point = [&](int64_t p) {
        double k = m[p] * rf[p];
        if (gf) k = k + gf[p];
        const double s = a * k, t = b * k;
        const double base = af ? af[p] : 0.0;
        if (wf) wf[p] = vf ? vf[p] + s : s;
        of[p] = af ? base + t : t;
    };
    if constexpr (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = t0; i < pairs; i += step) {
            const int64_t p = 2 * i;
            const double2 mm = ld2(m + p), rr = ld2(rf + p);
            double2 k = make_double2(mm.x * rr.x, mm.y * rr.y);
            if (gf) {
                const double2 gg = ld2(gf + p);
                k = make_double2(k.x + gg.x, k.y + gg.y);
            }
            const double2 t = make_double2(b * k.x, b * k.y);
            double2 o = t;
            if (af) {   // (read before w is written: acc_out may be v)
                const double2 base = ld2(af + p);
                o = make_double2(base.x + t.x, base.y + t.y);
            }
            if (wf) {
                double2 s = make_double2(a * k.x, a * k.y);
                if (vf) {
                    const double2 vv = ld2(vf + p);
                    s = make_double2(vv.x + s.x, vv.y + s.y);
                }
                st2(wf + p, s);
            }
            st2(of + p, o);
        }
        if ((n & 1) && t0 == 0) point(n - 1);
    } else {
        for (int64_t p = t0; p < n; p += step) point(p);
    }
    if (f == 0 && zero_p) {
        for (int64_t p = t0; p < n_p; p += step) zero_p[p] = 0.0;
        if (t0 == 0) *zero_t = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// The base flow and its tangent side by side (nekStab's ifbase = .true.: the nonlinear flow and the
// perturbation advance together): for a base state B and a perturbation u of nfld fields each, one tiled pass
// writes both local right-hand sides
//   rB_f = r_advdiff,f(B; U = B_vel)                                   (the bits of k_advdiff_rhs<.., false>)
//   ru_f = r_advdiff,f(u; U = B_vel) - bm1 sum_{d<LDIM} u_d d_d B_f    (the bits of k_linconv_rhs<.., false>)
// The coordinates are staged and the factors formed once per group; B_f is staged once and its line sums
// feed the self-advection sum_d B_d d_d B_f, the diffusion flux of B and the production term.  The three flux
// tiles serve B and then u, so the footprint stays k_linconv_rhs's: lx1^2 + (LDIM + 2) nt doubles.  Only
// the production term waits in a register between the two halves of a field.  Every read of the field tiles
// lies before the field's last barrier, so the next field is staged without one of its own: four barriers
// per field, where the two kernels take three each.  Each output keeps the operand order of the kernel it
// restates.  The launch bounds ask for 4 waves per SIMD (128 VGPRs, as k_linconv_rhs reaches unasked): two
// 512-thread workgroups per CU at lx1 = 8 in 3-D, for about ten spilled registers.
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__((tile_threads<LDIM, NX>()), 4) void k_burgers_tangent_rhs(
    int64_t nel, int epb, int nfld, const double* __restrict__ Dg, const double* __restrict__ wg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ B, int64_t b_stride, const double* __restrict__ kappa, const double* __restrict__ u,
    int64_t u_stride, double* __restrict__ rB, int64_t rb_stride, double* __restrict__ ru, int64_t ru_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    // two field tiles: U, the perturbation field being differentiated, and Bt, the base field; the flux tiles
    // hold the fluxes of B, then of u
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);
    const int tid = t.tid;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        const double jacmi = 1.0 / jac;
        const double bm = jac * t.wt;
        double Ub[LDIM];       // the advecting velocity B_d
        double P[LDIM];        // the velocity perturbation u_d
#pragma unroll
        for (int d = 0; d < LDIM; ++d) {
            Ub[d] = live ? B[d * b_stride + p] : 0.0;
            P[d] = live ? u[d * u_stride + p] : 0.0;
        }
        for (int f = 0; f < nfld; ++f) {
            // (every lane differentiated the previous field before that field's last barrier)
            if (live) {
                t.U[tid] = u[f * u_stride + p];
                t.Bt[tid] = B[f * b_stride + p];
            }
            __syncthreads();   // (and every lane has formed its factors / read the previous fluxes of u)
            double advB = 0.0, advu = 0.0, prod = 0.0;
            const double kb = live ? -kappa[f] * bm : 0.0;
            if (live) {
                // field_fluxes of B_f, spelled out: the production term rides on the derivatives of the base state
                double dB[LDIM], G[LDIM];
                physical_gradient<LDIM, NX>(t.q, t.Bt, g, jacmi, dB);
#pragma unroll
                for (int d = 0; d < LDIM; ++d) {
                    G[d] = kb * dB[d];
                    advB = advB + Ub[d] * dB[d];
                    prod = d == 0 ? P[0] * dB[d] : prod + P[d] * dB[d];
                }
                write_fluxes(t, g, jacmi, G);
            }
            __syncthreads();
            if (live) rB[f * rb_stride + p] = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z) - bm * advB;
            __syncthreads();   // the fluxes of B are read
            if (live) advu = field_fluxes<false>(t, t.U, g, jacmi, bm, kb, Ub);
            __syncthreads();
            if (live)
                ru[f * ru_stride + p] = (transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z) - bm * advu) - bm * prod;
        }
    }
}

// ------------------------------------------------------------------------------------------
// One RK4 stage of the base flow under a harmonic forcing and, optionally, of its tangent in the same launch
// (grid.y = field).  Base half, per point, in this order, no contraction:
//   k = m r [+ g0] [+ c gc] [+ s gs]      w = v + a k      acc' = (first ? v : acc) + b k
// c, s: the cos and sin of the stage's phase, formed by the host.  Tangent half: k_rk4_stage without g, on
// its own v, r, acc, w and acc'; a NULL r skips it.  A block runs the base half of its points, then the
// tangent half (m comes from the cache the second time).  The NULL conventions, the zeroing and VEC as in
// k_rk4_stage.
// ------------------------------------------------------------------------------------------
struct StageHalf {
    const double *v, *r, *acc;
    double *w, *ao;
    int64_t v_stride, r_stride, acc_stride, w_stride, ao_stride;
    double *zero_p, *zero_t;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_orbit_stage(int64_t n, const double* __restrict__ m, StageHalf hb,
                                                          const double* __restrict__ g0, const double* __restrict__ gc,
                                                          const double* __restrict__ gs, int64_t g_stride, double c,
                                                          double s, StageHalf ht, double a, double b, int first,
                                                          int64_t n_p) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const double* g0f = g0 ? g0 + f * g_stride : nullptr;
    const double* gcf = gc ? gc + f * g_stride : nullptr;
    const double* gsf = gs ? gs + f * g_stride : nullptr;
    const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
    for (int half = 0; half < 2; ++half) {
        const StageHalf& h = half ? ht : hb;
        if (!h.r) continue;   // no tangent half
        const bool forced = half == 0;
        const double* vf = h.v ? h.v + f * h.v_stride : nullptr;
        const double* rf = h.r + f * h.r_stride;
        const double* af = first ? vf : h.acc + f * h.acc_stride;
        double* wf = h.w ? h.w + f * h.w_stride : nullptr;
        double* of = h.ao + f * h.ao_stride;
        auto point = [&](int64_t p) {
            double k = m[p] * rf[p];
            if (forced) {
                if (g0f) k = k + g0f[p];
                if (gcf) k = k + c * gcf[p];
                if (gsf) k = k + s * gsf[p];
            }
            const double sa = a * k, t = b * k;
            const double base = af ? af[p] : 0.0;
            if (wf) wf[p] = vf ? vf[p] + sa : sa;
            of[p] = af ? base + t : t;
        };
        if constexpr (VEC) {
            const int64_t pairs = n / 2;
            for (int64_t i = t0; i < pairs; i += step) {
                const int64_t p = 2 * i;
                const double2 mm = ld2(m + p), rr = ld2(rf + p);
                double2 k = make_double2(mm.x * rr.x, mm.y * rr.y);
                if (forced) {
                    if (g0f) {
                        const double2 gg = ld2(g0f + p);
                        k = make_double2(k.x + gg.x, k.y + gg.y);
                    }
                    if (gcf) {
                        const double2 gg = ld2(gcf + p);
                        k = make_double2(k.x + c * gg.x, k.y + c * gg.y);
                    }
                    if (gsf) {
                        const double2 gg = ld2(gsf + p);
                        k = make_double2(k.x + s * gg.x, k.y + s * gg.y);
                    }
                }
                const double2 t = make_double2(b * k.x, b * k.y);
                double2 o = t;
                if (af) {   // (read before w is written: acc_out may be v)
                    const double2 base = ld2(af + p);
                    o = make_double2(base.x + t.x, base.y + t.y);
                }
                if (wf) {
                    double2 sa = make_double2(a * k.x, a * k.y);
                    if (vf) {
                        const double2 vv = ld2(vf + p);
                        sa = make_double2(vv.x + sa.x, vv.y + sa.y);
                    }
                    st2(wf + p, sa);
                }
                st2(of + p, o);
            }
            if ((n & 1) && t0 == 0) point(n - 1);
        } else {
            for (int64_t p = t0; p < n; p += step) point(p);
        }
        if (f == 0 && h.zero_p) {
            for (int64_t p = t0; p < n_p; p += step) h.zero_p[p] = 0.0;
            if (t0 == 0) *h.zero_t = 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The linearised convection of a complex (re/im pair) perturbation about a real base state B: B does not mix
// the halves, so one tiled pass writes
//   r_re = k_linconv_rhs<.., ADJ>(u_re; B)      r_im = k_linconv_rhs<.., ADJ>(u_im; B)      (the same bits)
// where the resolvent's Horner pass would launch k_linconv_rhs twice.  Per element group the coordinates are
// staged, the factors formed and Ub[d] read once.  Forward: B_f is staged once per field, its LDIM physical
// derivatives wait in registers and close the production term of both halves with P_re[d], P_im[d].  Adjoint:
// the first sweep stages and differentiates each B_f' once and accumulates P_re[d] and P_im[d] in the
// ascending order of k_linconv_rhs.  The field tile and the three flux tiles serve the re half and then the
// im half, as k_burgers_tangent_rhs reuses them for B and then u: the im half is staged while the re fluxes
// are summed, and every read of the field tiles lies before the field's last barrier, so the next field is
// staged without a barrier of its own: four barriers per field, where two launches take six.  LDS as
// k_linconv_rhs: lx1^2 + (LDIM + 2) nt doubles.  Streams per point at LDIM = 3, nfld = 4: 3 + 4 + 8 + 8 = 23
// doubles where two launches move 30.  Each output keeps the operand order of k_linconv_rhs.
// NKV_CRHS_WAVES: the waves per SIMD the launch bounds ask for (0: none asked); tools/bench_coupled_resolvent.py
// measured both and the default is the faster (CHANGELOG).
// ------------------------------------------------------------------------------------------
#ifndef NKV_CRHS_WAVES
#define NKV_CRHS_WAVES 4
#endif
#if NKV_CRHS_WAVES > 0
#define NKV_CRHS_BOUNDS(T) __launch_bounds__((T), NKV_CRHS_WAVES)
#else
#define NKV_CRHS_BOUNDS(T) __launch_bounds__((T))
#endif

template <int LDIM, int NX, bool ADJ>
__global__ NKV_CRHS_BOUNDS((tile_threads<LDIM, NX>())) void k_linconv_crhs(
    int64_t nel, int epb, int nfld, const double* __restrict__ Dg, const double* __restrict__ wg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ B, int64_t b_stride, const double* __restrict__ kappa, const double* __restrict__ u_re,
    const double* __restrict__ u_im, int64_t u_stride, double* __restrict__ r_re, double* __restrict__ r_im,
    int64_t r_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    // two field tiles: U, the field being differentiated (re, then im), and Bt, the base field being
    // differentiated; the flux tiles hold the fluxes of the re, then of the im half
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);
    const int tid = t.tid;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        const double jacmi = 1.0 / jac;
        const double bm = jac * t.wt;
        double Ub[LDIM];       // the advecting velocity B_d
        double Pr[LDIM];       // forward: the velocity perturbation u_re,d; adjoint: sum_f' u_re,f' d_d B_f'
        double Pi[LDIM];       // ... of the im half
#pragma unroll
        for (int d = 0; d < LDIM; ++d) {
            Ub[d] = live ? B[d * b_stride + p] : 0.0;
            Pr[d] = (!ADJ && live) ? u_re[d * u_stride + p] : 0.0;
            Pi[d] = (!ADJ && live) ? u_im[d * u_stride + p] : 0.0;
        }
        if constexpr (ADJ) {
            for (int f = 0; f < nfld; ++f) {
                double* T = (f & 1) ? t.Bt : t.U;   // the tile written two fields ago: a barrier lies between
                if (live) T[tid] = B[f * b_stride + p];
                __syncthreads();
                if (live) {
                    // presweep_field spelled out: one differentiation of B_f' serves both halves
                    double db[LDIM];
                    physical_gradient<LDIM, NX>(t.q, T, g, jacmi, db);
                    const double ur = u_re[f * u_stride + p], ui = u_im[f * u_stride + p];
#pragma unroll
                    for (int d = 0; d < LDIM; ++d) {
                        Pr[d] = f == 0 ? ur * db[d] : Pr[d] + ur * db[d];
                        Pi[d] = f == 0 ? ui * db[d] : Pi[d] + ui * db[d];
                    }
                }
            }
            __syncthreads();   // every lane is done reading the last base field
        }
        for (int f = 0; f < nfld; ++f) {
            // (every lane differentiated the previous field before that field's last barrier)
            if (live) {
                t.U[tid] = u_re[f * u_stride + p];
                if constexpr (!ADJ) t.Bt[tid] = B[f * b_stride + p];
            }
            __syncthreads();   // (and every lane has formed its factors / read the previous fluxes)
            const double kb = live ? -kappa[f] * bm : 0.0;
            double prod_re = 0.0, prod_im = 0.0;
            double adv = 0.0;
            if (live) {
                if constexpr (!ADJ) {
                    double db[LDIM];
                    physical_gradient<LDIM, NX>(t.q, t.Bt, g, jacmi, db);
#pragma unroll
                    for (int d = 0; d < LDIM; ++d) {
                        prod_re = d == 0 ? Pr[0] * db[d] : prod_re + Pr[d] * db[d];
                        prod_im = d == 0 ? Pi[0] * db[d] : prod_im + Pi[d] * db[d];
                    }
                } else {
#pragma unroll
                    for (int d = 0; d < LDIM; ++d)
                        if (f == d) {
                            prod_re = Pr[d];
                            prod_im = Pi[d];
                        }
                }
                adv = field_fluxes<ADJ>(t, t.U, g, jacmi, bm, kb, Ub);
            }
            __syncthreads();
            if (live) {
                const double acc = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z);
                if constexpr (ADJ)
                    r_re[f * r_stride + p] = f < LDIM ? acc - bm * prod_re : acc;
                else
                    r_re[f * r_stride + p] = (acc - bm * adv) - bm * prod_re;
                t.U[tid] = u_im[f * u_stride + p];   // the re half was differentiated before the barrier above
            }
            __syncthreads();   // the fluxes of the re half are read, the im half is staged
            if (live) adv = field_fluxes<ADJ>(t, t.U, g, jacmi, bm, kb, Ub);
            __syncthreads();
            if (live) {
                const double acc = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z);
                if constexpr (ADJ)
                    r_im[f * r_stride + p] = f < LDIM ? acc - bm * prod_im : acc;
                else
                    r_im[f * r_stride + p] = (acc - bm * adv) - bm * prod_im;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// The backward sweep of a checkpointed adjoint (orbit.py): while the adjoint runs backwards through one segment
// of the orbit, the segment before it is recomputed forwards.  For the base state X being advanced, a stored
// stage state S and the adjoint variable u of nfld fields each, one tiled pass writes both local right-hand
// sides
//   rX_f = r_advdiff,f(X; U = X_vel)                                   (the bits of k_advdiff_rhs<.., false>)
//   ru_f = r_advdiff,adj,f(u; U = S_vel) - [f < LDIM] bm1 sum_f' u_f' d_f S_f'   (k_linconv_rhs<.., true>)
// The coordinates are staged and the factors formed once per group.  First the X sweep (field tile and LDIM
// flux tiles), then the adjoint: the sweep over the fields of S that accumulates sum_f' u_f' d_d S_f' in LDIM
// registers, then the sweep over u through the same flux tiles.  Every staged field alternates between the
// two field tiles (U, Bt) through all three sweeps, so a field is staged while lanes may still differentiate
// the one before it and a tile is rewritten only with a barrier behind its last reader: two barriers per
// field in the X sweep and in the sweep over u, one in the sweep over S, 2 + 5 nfld per group where the two
// kernels take 4 + 7 nfld.  LDS as k_linconv_rhs: lx1^2 + (LDIM + 2) nt doubles, sized at the launch, below
// 64 KiB (no attribute to raise).  Each output keeps the operand order of the kernel it restates.  Streams per
// point at LDIM = 3, nfld = 4: 3 + 4 + 4 + 4 + 8 = 23 doubles where the two launches move 14 + 15 = 29.
// NKV_BWD_WAVES: the waves per SIMD the launch bounds ask for (0: none asked).  At lx1 = 8 in 3-D the kernel
// takes 126 VGPRs at four waves either way (the same code); at odd lx1 in 3-D the request costs two or three
// spilled registers where 130-132 VGPRs would leave three waves, the trade k_burgers_tangent_rhs measured.
// ------------------------------------------------------------------------------------------
#ifndef NKV_BWD_WAVES
#define NKV_BWD_WAVES 4
#endif
#if NKV_BWD_WAVES > 0
#define NKV_BWD_BOUNDS(T) __launch_bounds__((T), NKV_BWD_WAVES)
#else
#define NKV_BWD_BOUNDS(T) __launch_bounds__((T))
#endif

template <int LDIM, int NX>
__global__ NKV_BWD_BOUNDS((tile_threads<LDIM, NX>())) void k_burgers_backward_rhs(
    int64_t nel, int epb, int nfld, const double* __restrict__ Dg, const double* __restrict__ wg,
    const double* __restrict__ xm, const double* __restrict__ ym, const double* __restrict__ zm,
    const double* __restrict__ Xs, int64_t x_stride, const double* __restrict__ Sb, int64_t s_stride,
    const double* __restrict__ kappa, const double* __restrict__ u, int64_t u_stride, double* __restrict__ rX,
    int64_t rx_stride, double* __restrict__ ru, int64_t ru_stride) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    // two field tiles, U and Bt: staged fields alternate between them; the flux tiles hold the fluxes of X,
    // then of u
    const TileFrame<LDIM, NX> t(lds, epb, Dg, wg);
    const int tid = t.tid;
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < nel; e0 += (int64_t)gridDim.x * epb) {
        int64_t p;
        double g[3][3], jac;
        const bool live = t.begin_group(e0, nel, xm, ym, zm, p, g, jac);
        const double jacmi = 1.0 / jac;
        const double bm = jac * t.wt;
        int stage = 0;         // fields staged so far in this group: the next one goes to tile (stage & 1)
        double Ub[LDIM];       // the advecting velocity: X_d, then S_d
        // ---- the X sweep: k_advdiff_rhs<.., false> with u = U = X ----
#pragma unroll
        for (int d = 0; d < LDIM; ++d) Ub[d] = live ? Xs[d * x_stride + p] : 0.0;
        for (int f = 0; f < nfld; ++f, ++stage) {
            double* T = (stage & 1) ? t.Bt : t.U;   // last read two fields ago: a barrier lies between
            if (live) T[tid] = Xs[f * x_stride + p];
            __syncthreads();   // (every lane has formed its factors / read the previous field's fluxes)
            double adv = 0.0;
            if (live) adv = field_fluxes<false>(t, T, g, jacmi, bm, -kappa[f] * bm, Ub);
            __syncthreads();
            if (live) rX[f * rx_stride + p] = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z) - bm * adv;
        }
        // ---- the adjoint: k_linconv_rhs<.., true> of u about S ----
        double P[LDIM];        // sum_f' u_f' d_d S_f'
#pragma unroll
        for (int d = 0; d < LDIM; ++d) {
            Ub[d] = live ? Sb[d * s_stride + p] : 0.0;
            P[d] = 0.0;
        }
        for (int f = 0; f < nfld; ++f, ++stage) {
            double* T = (stage & 1) ? t.Bt : t.U;
            if (live) T[tid] = Sb[f * s_stride + p];
            __syncthreads();
            if (live) presweep_field<LDIM, NX>(t.q, T, g, jacmi, u[f * u_stride + p], f == 0, P);
        }
        for (int f = 0; f < nfld; ++f, ++stage) {
            double* T = (stage & 1) ? t.Bt : t.U;
            if (live) T[tid] = u[f * u_stride + p];
            __syncthreads();   // (every lane has read the fluxes of the field before: of X the first time)
            double prod = 0.0;
            if (live) {
                field_fluxes<true>(t, T, g, jacmi, bm, -kappa[f] * bm, Ub);
#pragma unroll
                for (int d = 0; d < LDIM; ++d)
                    if (f == d) prod = P[d];
            }
            __syncthreads();
            if (live) {
                const double acc = transposed_line_sums<LDIM, NX>(t.q, t.X, t.Y, t.Z);
                ru[f * ru_stride + p] = f < LDIM ? acc - bm * prod : acc;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// The host side the tiled entries share.
// ------------------------------------------------------------------------------------------

// The launcher of every tiled kernel: NF field tiles behind the LDIM coordinate tiles size the dynamic LDS
// (lx1^2 + (LDIM + NF) nt doubles, below 64 KiB: no attribute to raise); args follow (nel, epb).
template <int LDIM, int NX, int NF, typename Kernel, typename... Args>
void launch_tiled(Kernel kernel, int64_t nel, hipStream_t st, Args... args) {
    constexpr int pts = tile_pts<LDIM, NX>();
    const int epb = tile_epb(pts);
    static_assert(NF >= 0 && NF <= 2, "a tiled kernel has at most two field tiles");
    const size_t lds = sizeof(double) * ((size_t)NX * NX + (size_t)(LDIM + NF) * epb * pts);
    static_assert(sizeof(double) * (10 * 10 + 4 * 1000) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    static_assert(sizeof(double) * (10 * 10 + 5 * 1000) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    const int64_t groups = (nel + epb - 1) / epb;
    const int grid = (int)std::min<int64_t>(groups, 16384);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(tile_threads<LDIM, NX>()), lds, st, nel, epb, args...);
}

// The lx1 x ldim dispatch: calls f(ldim, lx1) with both as integral constants.  check_mesh_args has let
// through ldim = 2, 3 and lx1 = 2..10 only.
template <typename F>
void dispatch_tile(int lx1, int ldim, F&& f) {
#define NKV_AD_CASE(NX)                                                                          \
    case NX:                                                                                     \
        if (ldim == 3) f(std::integral_constant<int, 3>{}, std::integral_constant<int, NX>{});   \
        else f(std::integral_constant<int, 2>{}, std::integral_constant<int, NX>{});             \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_AD_CASE) }
#undef NKV_AD_CASE
}

// Whether the spans of two operands of nfld fields (n points each, a stride apart) meet.
inline bool spans_meet(const double* p, int64_t ps, const double* o, int64_t os, int nfld, int64_t n) {
    const double* pe = p + (int64_t)(nfld - 1) * ps + n;
    const double* oe = o + (int64_t)(nfld - 1) * os + n;
    return p < oe && o < pe;
}

// What every tiled entry checks first: the layout, the mesh arguments and the four arrays all of them read.
// *nel: the elements of this shard; 0 for an empty shard (more ranks than elements), which has nothing to
// touch and whose pointers are not looked at: the entry returns NKV_OK.
inline int check_tiled_entry(const char* who, const nkv_layout* L, int lx1, int ldim, const double* D, const double* w,
                             const double* xm, const double* ym, const double* zm, int64_t* nel) {
    *nel = 0;
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;
    CHECK(check_mesh_args(who, L, lx1, ldim, zm));
    CHECK(need(D, who, "D"));
    CHECK(need(w, who, "w"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    *nel = L->n_v / (ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1);
    return NKV_OK;
}

}  // namespace

extern "C" {

int nkv_advdiff_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, const double* U, int64_t U_stride, const double* kappa,
                    const double* u, int nfld, int64_t u_stride, double* r, int64_t r_stride, int adjoint,
                    void* stream) {
    static const char who[] = "advdiff_rhs";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    if (nfld < 1) return fail(NKV_EINVAL, "%s: nfld=%d < 1", who, nfld);
    if (U_stride < L->n_v || u_stride < L->n_v || r_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: strides U_stride=%lld u_stride=%lld r_stride=%lld below n_v=%lld", who,
                    (long long)U_stride, (long long)u_stride, (long long)r_stride, (long long)L->n_v);
    CHECK(need(U, who, "U"));
    CHECK(need(kappa, who, "kappa"));
    CHECK(need(u, who, "u"));
    CHECK(need(r, who, "r"));
    if (u == r) return fail(NKV_EINVAL, "%s cannot run in place (r is u)", who);
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        auto kernel = adjoint ? k_advdiff_rhs<LD, NX, true> : k_advdiff_rhs<LD, NX, false>;
        launch_tiled<LD, NX, 1>(kernel, nel, S(stream), nfld, D, w, xm, ym, zm, U, U_stride, kappa, u, u_stride, r,
                                r_stride);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_advdiff_bm1(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, double* bm1, void* stream) {
    static const char who[] = "advdiff_bm1";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    CHECK(need(bm1, who, "bm1"));
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        launch_tiled<LD, NX, 0>(k_advdiff_bm1<LD, NX>, nel, S(stream), D, w, xm, ym, zm, bm1);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_advdiff_stage(const nkv_layout* L, const double* v, int64_t v_stride, const double* minv, const double* r,
                      int64_t r_stride, double c, double* w, int64_t w_stride, int nfld, int zero_rest,
                      void* stream) {
    static const char who[] = "advdiff_stage";
    CHECK(check_layout(L));
    const int64_t n = L->n_v;
    if (n == 0) return NKV_OK;   // an empty shard: nothing to touch
    if (nfld < 1 || nfld > 65535) return fail(NKV_EINVAL, "%s: nfld=%d outside 1..65535", who, nfld);
    if ((v && v_stride < n) || r_stride < n || w_stride < n)
        return fail(NKV_EINVAL, "%s: strides v_stride=%lld r_stride=%lld w_stride=%lld below n_v=%lld", who,
                    (long long)v_stride, (long long)r_stride, (long long)w_stride, (long long)n);
    CHECK(need(minv, who, "minv"));
    CHECK(need(r, who, "r"));
    CHECK(need(w, who, "w"));
    if (!std::isfinite(c)) return fail(NKV_EINVAL, "%s: c=%g", who, c);
    if (zero_rest && (nfld != L->n_wf || w_stride != L->sv))
        return fail(NKV_EINVAL, "%s: zero_rest needs w to be a state vector (nfld=%d, n_wf=%d, w_stride=%lld, sv=%lld)",
                    who, nfld, L->n_wf, (long long)w_stride, (long long)L->sv);
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = a16(minv) && a16(r) && a16(w) && (!v || (a16(v) && v_stride % 2 == 0)) && r_stride % 2 == 0 &&
                     w_stride % 2 == 0 && n >= 2;
    double* zp = zero_rest ? w + (int64_t)L->n_wf * L->sv : nullptr;
    double* zt = zero_rest ? w + rows_of(L) : nullptr;
    const dim3 grid(grid_for(vec ? n / 2 : n, 1024), nfld);
    if (vec)
        hipLaunchKernelGGL(k_advdiff_stage<true>, grid, dim3(kThreads), 0, S(stream), n, v, v_stride, minv, r, r_stride, c,
                           w, w_stride, zp, L->n_p, zt);
    else
        hipLaunchKernelGGL(k_advdiff_stage<false>, grid, dim3(kThreads), 0, S(stream), n, v, v_stride, minv, r, r_stride,
                           c, w, w_stride, zp, L->n_p, zt);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_advdiff_cstage(const nkv_layout* L, const double* v_re, const double* v_im, int64_t v_stride,
                       const double* minv, const double* r_re, const double* r_im, int64_t r_stride,
                       const double* s_re, const double* s_im, int64_t s_stride, const double* f_re,
                       const double* f_im, int64_t f_stride, double omega, double c, double* w_re, double* w_im,
                       int64_t w_stride, int nfld, int zero_rest, void* stream) {
    static const char who[] = "advdiff_cstage";
    CHECK(check_layout(L));
    if (L->n_v == 0) return NKV_OK;   // an empty shard: nothing to touch
    if (L->n_v % 2) return fail(NKV_EINVAL, "%s: n_v=%lld is odd: L is the layout of re/im pair vectors", who,
                                (long long)L->n_v);
    const int64_t n = L->n_v / 2;
    if (nfld < 1 || nfld > 65535) return fail(NKV_EINVAL, "%s: nfld=%d outside 1..65535", who, nfld);
    if (!v_re != !v_im) return fail(NKV_EINVAL, "%s: v_re and v_im are both NULL or neither", who);
    if (!f_re != !f_im) return fail(NKV_EINVAL, "%s: f_re and f_im are both NULL or neither", who);
    if ((v_re && v_stride < n) || (f_re && f_stride < n) || r_stride < n || s_stride < n || w_stride < n)
        return fail(NKV_EINVAL,
                    "%s: strides v_stride=%lld r_stride=%lld s_stride=%lld f_stride=%lld w_stride=%lld below n_v/2=%lld",
                    who, (long long)v_stride, (long long)r_stride, (long long)s_stride, (long long)f_stride,
                    (long long)w_stride, (long long)n);
    CHECK(need(minv, who, "minv"));
    CHECK(need(r_re, who, "r_re"));
    CHECK(need(r_im, who, "r_im"));
    CHECK(need(s_re, who, "s_re"));
    CHECK(need(s_im, who, "s_im"));
    CHECK(need(w_re, who, "w_re"));
    CHECK(need(w_im, who, "w_im"));
    if (!std::isfinite(c) || !std::isfinite(omega)) return fail(NKV_EINVAL, "%s: c=%g omega=%g", who, c, omega);
    // w may be v (pointwise) and nothing else: the span of every input half against the span of each half of w
    auto span = [&](const double* p, int64_t stride) { return p + (int64_t)(nfld - 1) * stride + n; };
    auto meets_w = [&](const double* p, int64_t stride) {
        if (!p) return false;
        const double* e = span(p, stride);
        return (p < span(w_re, w_stride) && w_re < e) || (p < span(w_im, w_stride) && w_im < e);
    };
    if (meets_w(minv, 0) || meets_w(r_re, r_stride) || meets_w(r_im, r_stride) || meets_w(s_re, s_stride) ||
        meets_w(s_im, s_stride) || meets_w(f_re, f_stride) || meets_w(f_im, f_stride))
        return fail(NKV_EINVAL, "%s: w overlaps minv, r, s or f (only v may be w)", who);
    // the halves of w against each other: field i's re against field j's im, d + (j - i) w_stride apart
    const int64_t d = w_im < w_re ? w_re - w_im : w_im - w_re, k = d / w_stride, rem = d % w_stride;
    if (d < n || (rem < n && k >= 1 && k <= nfld - 1) || (w_stride - rem < n && k + 1 <= nfld - 1))
        return fail(NKV_EINVAL, "%s: the halves of w overlap", who);
    if (zero_rest && (nfld != L->n_wf || w_stride != L->sv || w_im != w_re + n))
        return fail(NKV_EINVAL,
                    "%s: zero_rest needs w to be a pair state vector (nfld=%d, n_wf=%d, w_stride=%lld, sv=%lld, "
                    "w_im = w_re + n_v/2)", who, nfld, L->n_wf, (long long)w_stride, (long long)L->sv);
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = n >= 2 && a16(minv) && a16(r_re) && a16(r_im) && a16(s_re) && a16(s_im) && a16(w_re) && a16(w_im) &&
                     r_stride % 2 == 0 && s_stride % 2 == 0 && w_stride % 2 == 0 &&
                     (!v_re || (a16(v_re) && a16(v_im) && v_stride % 2 == 0)) &&
                     (!f_re || (a16(f_re) && a16(f_im) && f_stride % 2 == 0));
    double* zp = zero_rest ? w_re + (int64_t)L->n_wf * L->sv : nullptr;
    double* zt = zero_rest ? w_re + rows_of(L) : nullptr;
    const dim3 grid(grid_for(vec ? n / 2 : n, 1024), nfld);
    if (vec)
        hipLaunchKernelGGL(k_advdiff_cstage<true>, grid, dim3(kThreads), 0, S(stream), n, v_re, v_im, v_stride, minv, r_re,
                           r_im, r_stride, s_re, s_im, s_stride, f_re, f_im, f_stride, omega, c, w_re, w_im, w_stride, zp,
                           L->n_p, zt);
    else
        hipLaunchKernelGGL(k_advdiff_cstage<false>, grid, dim3(kThreads), 0, S(stream), n, v_re, v_im, v_stride, minv, r_re,
                           r_im, r_stride, s_re, s_im, s_stride, f_re, f_im, f_stride, omega, c, w_re, w_im, w_stride, zp,
                           L->n_p, zt);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_linconv_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                    const double* u, int nfld, int64_t u_stride, double* r, int64_t r_stride, int adjoint,
                    void* stream) {
    static const char who[] = "linconv_rhs";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    if (nfld < ldim) return fail(NKV_EINVAL, "%s: nfld=%d < ldim=%d (the base state's first ldim fields advect)", who,
                                 nfld, ldim);
    if (B_stride < L->n_v || u_stride < L->n_v || r_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: strides B_stride=%lld u_stride=%lld r_stride=%lld below n_v=%lld", who,
                    (long long)B_stride, (long long)u_stride, (long long)r_stride, (long long)L->n_v);
    CHECK(need(B, who, "B"));
    CHECK(need(kappa, who, "kappa"));
    CHECK(need(u, who, "u"));
    CHECK(need(r, who, "r"));
    // r is written field by field while later fields of u and B are still to be read: no overlap of the spans
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        return spans_meet(p, ps, o, os, nfld, L->n_v);
    };
    if (meets(u, u_stride, r, r_stride) || meets(B, B_stride, r, r_stride))
        return fail(NKV_EINVAL, "%s: r overlaps u or B", who);
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        auto kernel = adjoint ? k_linconv_rhs<LD, NX, true> : k_linconv_rhs<LD, NX, false>;
        launch_tiled<LD, NX, 2>(kernel, nel, S(stream), nfld, D, w, xm, ym, zm, B, B_stride, kappa, u, u_stride, r,
                                r_stride);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_linconv_crhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                     const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                     const double* u_re, const double* u_im, int nfld, int64_t u_stride, double* r_re, double* r_im,
                     int64_t r_stride, int adjoint, void* stream) {
    static const char who[] = "linconv_crhs";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    if (nfld < ldim) return fail(NKV_EINVAL, "%s: nfld=%d < ldim=%d (the base state's first ldim fields advect)", who,
                                 nfld, ldim);
    if (B_stride < L->n_v) return fail(NKV_EINVAL, "%s: B_stride=%lld below n_v=%lld", who, (long long)B_stride,
                                       (long long)L->n_v);
    if (u_stride < L->n_v) return fail(NKV_EINVAL, "%s: u_stride=%lld below n_v=%lld", who, (long long)u_stride,
                                       (long long)L->n_v);
    if (r_stride < L->n_v) return fail(NKV_EINVAL, "%s: r_stride=%lld below n_v=%lld", who, (long long)r_stride,
                                       (long long)L->n_v);
    CHECK(need(B, who, "B"));
    CHECK(need(kappa, who, "kappa"));
    CHECK(need(u_re, who, "u_re"));
    CHECK(need(u_im, who, "u_im"));
    CHECK(need(r_re, who, "r_re"));
    CHECK(need(r_im, who, "r_im"));
    // both results are written field by field while later fields of u_re, u_im and B are still to be read.  The
    // halves of a pair vector interleave (field f's im half lies between the re halves of f and f + 1), so
    // where the whole spans meet the field segments decide
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        const int64_t n = L->n_v;
        if (!spans_meet(p, ps, o, os, nfld, n)) return false;
        for (int i = 0; i < nfld; ++i)
            for (int j = 0; j < nfld; ++j) {
                const double *a = p + (int64_t)i * ps, *b = o + (int64_t)j * os;
                if (a < b + n && b < a + n) return true;
            }
        return false;
    };
    if (meets(r_re, r_stride, r_im, r_stride)) return fail(NKV_EINVAL, "%s: r_re overlaps r_im", who);
    if (meets(u_re, u_stride, r_re, r_stride) || meets(u_im, u_stride, r_re, r_stride) ||
        meets(B, B_stride, r_re, r_stride))
        return fail(NKV_EINVAL, "%s: r_re overlaps u_re, u_im or B", who);
    if (meets(u_re, u_stride, r_im, r_stride) || meets(u_im, u_stride, r_im, r_stride) ||
        meets(B, B_stride, r_im, r_stride))
        return fail(NKV_EINVAL, "%s: r_im overlaps u_re, u_im or B", who);
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        auto kernel = adjoint ? k_linconv_crhs<LD, NX, true> : k_linconv_crhs<LD, NX, false>;
        launch_tiled<LD, NX, 2>(kernel, nel, S(stream), nfld, D, w, xm, ym, zm, B, B_stride, kappa, u_re, u_im,
                                u_stride, r_re, r_im, r_stride);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_rk4_stage(const nkv_layout* L, const double* v, int64_t v_stride, const double* minv, const double* r,
                  int64_t r_stride, const double* g, int64_t g_stride, double a, double b, int first,
                  const double* acc, int64_t acc_stride, double* w, int64_t w_stride, double* acc_out,
                  int64_t ao_stride, int nfld, int zero_rest, void* stream) {
    static const char who[] = "rk4_stage";
    CHECK(check_layout(L));
    const int64_t n = L->n_v;
    if (n == 0) return NKV_OK;   // an empty shard: nothing to touch
    if (nfld < 1 || nfld > 65535) return fail(NKV_EINVAL, "%s: nfld=%d outside 1..65535", who, nfld);
    const bool need_v = (first || w) && v, need_acc = !first;   // v = NULL stands for zero
    if ((need_v && v_stride < n) || r_stride < n || (g && g_stride < n) || (need_acc && acc_stride < n) ||
        (w && w_stride < n) || ao_stride < n)
        return fail(NKV_EINVAL,
                    "%s: strides v_stride=%lld r_stride=%lld g_stride=%lld acc_stride=%lld w_stride=%lld "
                    "ao_stride=%lld below n_v=%lld", who, (long long)v_stride, (long long)r_stride, (long long)g_stride,
                    (long long)acc_stride, (long long)w_stride, (long long)ao_stride, (long long)n);
    CHECK(need(minv, who, "minv"));
    CHECK(need(r, who, "r"));
    CHECK(need(acc_out, who, "acc_out"));
    if (need_acc) CHECK(need(acc, who, "acc"));
    if (!std::isfinite(a) || !std::isfinite(b)) return fail(NKV_EINVAL, "%s: a=%g b=%g", who, a, b);
    // acc_out may be acc or v exactly (pointwise); otherwise no output span meets another operand's
    auto end = [&](const double* p, int64_t stride) { return p + (int64_t)(nfld - 1) * stride + n; };
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        return p && o && p < end(o, os) && o < end(p, ps);
    };
    const double* vv = need_v ? v : nullptr;
    const double* aa = need_acc ? acc : nullptr;
    auto out_bad = [&](const double* o, int64_t os, bool may_alias) {
        if (meets(minv, 0, o, os) || meets(r, r_stride, o, os) || meets(g, g_stride, o, os)) return true;
        if (meets(vv, v_stride, o, os) && !(may_alias && vv == o && v_stride == os)) return true;
        if (meets(aa, acc_stride, o, os) && !(may_alias && aa == o && acc_stride == os)) return true;
        return false;
    };
    if (out_bad(acc_out, ao_stride, true) || (w && (out_bad(w, w_stride, false) || meets(w, w_stride, acc_out, ao_stride))))
        return fail(NKV_EINVAL, "%s: w or acc_out overlaps an operand (only acc_out may be acc or v)", who);
    if (zero_rest && (nfld != L->n_wf || ao_stride != L->sv))
        return fail(NKV_EINVAL,
                    "%s: zero_rest needs acc_out to be a state vector (nfld=%d, n_wf=%d, ao_stride=%lld, sv=%lld)", who,
                    nfld, L->n_wf, (long long)ao_stride, (long long)L->sv);
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = n >= 2 && a16(minv) && a16(r) && r_stride % 2 == 0 && a16(acc_out) && ao_stride % 2 == 0 &&
                     (!need_v || (a16(v) && v_stride % 2 == 0)) && (!g || (a16(g) && g_stride % 2 == 0)) &&
                     (!need_acc || (a16(acc) && acc_stride % 2 == 0)) && (!w || (a16(w) && w_stride % 2 == 0));
    double* zp = zero_rest ? acc_out + (int64_t)L->n_wf * L->sv : nullptr;
    double* zt = zero_rest ? acc_out + rows_of(L) : nullptr;
    const dim3 grid(grid_for(vec ? n / 2 : n, 1024), nfld);
    if (vec)
        hipLaunchKernelGGL(k_rk4_stage<true>, grid, dim3(kThreads), 0, S(stream), n, vv, v_stride, minv, r, r_stride, g,
                           g_stride, a, b, first ? 1 : 0, aa, acc_stride, w, w_stride, acc_out, ao_stride, zp, L->n_p, zt);
    else
        hipLaunchKernelGGL(k_rk4_stage<false>, grid, dim3(kThreads), 0, S(stream), n, vv, v_stride, minv, r, r_stride, g,
                           g_stride, a, b, first ? 1 : 0, aa, acc_stride, w, w_stride, acc_out, ao_stride, zp, L->n_p, zt);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_burgers_tangent_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                            const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                            const double* u, int nfld, int64_t u_stride, double* r_B, int64_t rB_stride, double* r_u,
                            int64_t ru_stride, void* stream) {
    static const char who[] = "burgers_tangent_rhs";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    if (nfld < ldim) return fail(NKV_EINVAL, "%s: nfld=%d < ldim=%d (the base state's first ldim fields advect)", who,
                                 nfld, ldim);
    if (B_stride < L->n_v || u_stride < L->n_v || rB_stride < L->n_v || ru_stride < L->n_v)
        return fail(NKV_EINVAL, "%s: strides B_stride=%lld u_stride=%lld rB_stride=%lld ru_stride=%lld below n_v=%lld",
                    who, (long long)B_stride, (long long)u_stride, (long long)rB_stride, (long long)ru_stride,
                    (long long)L->n_v);
    CHECK(need(B, who, "B"));
    CHECK(need(kappa, who, "kappa"));
    CHECK(need(u, who, "u"));
    CHECK(need(r_B, who, "r_B"));
    CHECK(need(r_u, who, "r_u"));
    // both results are written field by field while later fields of u and B are still to be read
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        return spans_meet(p, ps, o, os, nfld, L->n_v);
    };
    if (meets(r_B, rB_stride, r_u, ru_stride)) return fail(NKV_EINVAL, "%s: r_B overlaps r_u", who);
    if (meets(u, u_stride, r_B, rB_stride) || meets(B, B_stride, r_B, rB_stride))
        return fail(NKV_EINVAL, "%s: r_B overlaps u or B", who);
    if (meets(u, u_stride, r_u, ru_stride) || meets(B, B_stride, r_u, ru_stride))
        return fail(NKV_EINVAL, "%s: r_u overlaps u or B", who);
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        launch_tiled<LD, NX, 2>(k_burgers_tangent_rhs<LD, NX>, nel, S(stream), nfld, D, w, xm, ym, zm, B, B_stride,
                                kappa, u, u_stride, r_B, rB_stride, r_u, ru_stride);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_burgers_backward_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                             const double* ym, const double* zm, const double* X, int64_t X_stride, const double* Sb,
                             int64_t S_stride, const double* kappa, const double* u, int nfld, int64_t u_stride,
                             double* r_X, int64_t rX_stride, double* r_u, int64_t ru_stride, void* stream) {
    static const char who[] = "burgers_backward_rhs";
    int64_t nel;
    CHECK(check_tiled_entry(who, L, lx1, ldim, D, w, xm, ym, zm, &nel));
    if (nel == 0) return NKV_OK;   // an empty shard
    if (nfld < ldim) return fail(NKV_EINVAL, "%s: nfld=%d < ldim=%d (the first ldim fields of X and S advect)", who,
                                 nfld, ldim);
    if (X_stride < L->n_v || S_stride < L->n_v || u_stride < L->n_v || rX_stride < L->n_v || ru_stride < L->n_v)
        return fail(NKV_EINVAL,
                    "%s: strides X_stride=%lld S_stride=%lld u_stride=%lld rX_stride=%lld ru_stride=%lld below n_v=%lld",
                    who, (long long)X_stride, (long long)S_stride, (long long)u_stride, (long long)rX_stride,
                    (long long)ru_stride, (long long)L->n_v);
    CHECK(need(X, who, "X"));
    CHECK(need(Sb, who, "S"));
    CHECK(need(kappa, who, "kappa"));
    CHECK(need(u, who, "u"));
    CHECK(need(r_X, who, "r_X"));
    CHECK(need(r_u, who, "r_u"));
    // both results are written field by field while later fields of X, S and u are still to be read; X and S
    // are only read and may be one state
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        return spans_meet(p, ps, o, os, nfld, L->n_v);
    };
    if (meets(r_X, rX_stride, r_u, ru_stride)) return fail(NKV_EINVAL, "%s: r_X overlaps r_u", who);
    if (meets(X, X_stride, r_X, rX_stride) || meets(Sb, S_stride, r_X, rX_stride) || meets(u, u_stride, r_X, rX_stride))
        return fail(NKV_EINVAL, "%s: r_X overlaps X, S or u", who);
    if (meets(X, X_stride, r_u, ru_stride) || meets(Sb, S_stride, r_u, ru_stride) || meets(u, u_stride, r_u, ru_stride))
        return fail(NKV_EINVAL, "%s: r_u overlaps X, S or u", who);
    dispatch_tile(lx1, ldim, [&](auto ld, auto nx) {
        constexpr int LD = decltype(ld)::value, NX = decltype(nx)::value;
        launch_tiled<LD, NX, 2>(k_burgers_backward_rhs<LD, NX>, nel, S(stream), nfld, D, w, xm, ym, zm, X, X_stride, Sb,
                                S_stride, kappa, u, u_stride, r_X, rX_stride, r_u, ru_stride);
    });
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_orbit_stage(const nkv_layout* L, const double* minv, const double* v, int64_t v_stride, const double* r,
                    int64_t r_stride, const double* g0, const double* gc, const double* gs, int64_t g_stride, double c,
                    double s, double a, double b, int first, const double* acc, int64_t acc_stride, double* w,
                    int64_t w_stride, double* acc_out, int64_t ao_stride, const double* tv, int64_t tv_stride,
                    const double* tr, int64_t tr_stride, const double* tacc, int64_t tacc_stride, double* tw,
                    int64_t tw_stride, double* tacc_out, int64_t tao_stride, int nfld, int zero_rest, void* stream) {
    static const char who[] = "orbit_stage";
    CHECK(check_layout(L));
    const int64_t n = L->n_v;
    if (n == 0) return NKV_OK;   // an empty shard: nothing to touch
    if (nfld < 1 || nfld > 65535) return fail(NKV_EINVAL, "%s: nfld=%d outside 1..65535", who, nfld);
    const bool tan = tr != nullptr;
    if (!tan && (tv || tacc || tw || tacc_out))
        return fail(NKV_EINVAL, "%s: tr is NULL (no tangent half) but another tangent pointer is not", who);
    if (zero_rest < 0 || zero_rest > 3 || ((zero_rest & 2) && !tan))
        return fail(NKV_EINVAL, "%s: zero_rest=%d (bit 0: acc_out, bit 1: tacc_out of a tangent half)", who, zero_rest);
    const bool forced = g0 || gc || gs;
    if (forced && g_stride < n) return fail(NKV_EINVAL, "%s: g_stride=%lld below n_v=%lld", who, (long long)g_stride,
                                            (long long)n);
    CHECK(need(minv, who, "minv"));
    CHECK(need(r, who, "r"));
    CHECK(need(acc_out, who, "acc_out"));
    if (tan) CHECK(need(tacc_out, who, "tacc_out"));
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c) || !std::isfinite(s))
        return fail(NKV_EINVAL, "%s: a=%g b=%g c=%g s=%g", who, a, b, c, s);
    const bool need_acc = !first;
    // one half as k_rk4_stage takes it: v = NULL stands for zero; v is read when first or w is given
    struct Half {
        const double *v, *r, *acc;
        double *w, *ao;
        int64_t vs, rs, as, ws, os;
    };
    Half H[2] = {{(first || w) ? v : nullptr, r, need_acc ? acc : nullptr, w, acc_out, v_stride, r_stride, acc_stride,
                  w_stride, ao_stride},
                 {(first || tw) ? tv : nullptr, tr, need_acc ? tacc : nullptr, tw, tacc_out, tv_stride, tr_stride,
                  tacc_stride, tw_stride, tao_stride}};
    const int nh = tan ? 2 : 1;
    for (int h = 0; h < nh; ++h) {
        const Half& x = H[h];
        if (need_acc) CHECK(need(x.acc, who, h ? "tacc" : "acc"));
        if ((x.v && x.vs < n) || x.rs < n || (x.acc && x.as < n) || (x.w && x.ws < n) || x.os < n)
            return fail(NKV_EINVAL,
                        "%s: %s half: strides v=%lld r=%lld acc=%lld w=%lld acc_out=%lld below n_v=%lld", who,
                        h ? "tangent" : "base", (long long)x.vs, (long long)x.rs, (long long)x.as, (long long)x.ws,
                        (long long)x.os, (long long)n);
    }
    // acc_out may be the acc or the v of its own half exactly (pointwise); otherwise no output span meets
    // another operand's, of either half
    auto end = [&](const double* p, int64_t stride) { return p + (int64_t)(nfld - 1) * stride + n; };
    auto meets = [&](const double* p, int64_t ps, const double* o, int64_t os) {
        return p && o && p < end(o, os) && o < end(p, ps);
    };
    auto out_bad = [&](int h, const double* o, int64_t os, bool may_alias) {
        if (meets(minv, 0, o, os) || meets(g0, g_stride, o, os) || meets(gc, g_stride, o, os) ||
            meets(gs, g_stride, o, os))
            return true;
        for (int k = 0; k < nh; ++k) {
            const Half& x = H[k];
            const bool own = may_alias && k == h;
            if (meets(x.r, x.rs, o, os)) return true;
            if (meets(x.v, x.vs, o, os) && !(own && x.v == o && x.vs == os)) return true;
            if (meets(x.acc, x.as, o, os) && !(own && x.acc == o && x.as == os)) return true;
        }
        return false;
    };
    bool bad = false;
    for (int h = 0; h < nh; ++h) {
        const Half& x = H[h];
        bad = bad || out_bad(h, x.ao, x.os, true) || (x.w && (out_bad(h, x.w, x.ws, false) || meets(x.w, x.ws, x.ao, x.os)));
    }
    if (tan)
        bad = bad || meets(H[0].ao, H[0].os, H[1].ao, H[1].os) || meets(H[0].ao, H[0].os, H[1].w, H[1].ws) ||
              meets(H[0].w, H[0].ws, H[1].ao, H[1].os) || meets(H[0].w, H[0].ws, H[1].w, H[1].ws);
    if (bad)
        return fail(NKV_EINVAL, "%s: w or acc_out overlaps an operand (only acc_out may be the acc or v of its half)", who);
    for (int h = 0; h < nh; ++h)
        if ((zero_rest & (1 << h)) && (nfld != L->n_wf || H[h].os != L->sv))
            return fail(NKV_EINVAL,
                        "%s: zero_rest needs %s to be a state vector (nfld=%d, n_wf=%d, ao_stride=%lld, sv=%lld)", who,
                        h ? "tacc_out" : "acc_out", nfld, L->n_wf, (long long)H[h].os, (long long)L->sv);
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    auto ok = [&](const void* p, int64_t stride) { return !p || (a16(p) && stride % 2 == 0); };
    bool vec = n >= 2 && a16(minv) && ok(g0, g_stride) && ok(gc, g_stride) && ok(gs, g_stride);
    StageHalf K[2] = {};
    for (int h = 0; h < nh; ++h) {
        const Half& x = H[h];
        vec = vec && ok(x.v, x.vs) && ok(x.r, x.rs) && ok(x.acc, x.as) && ok(x.w, x.ws) && ok(x.ao, x.os);
        const bool z = zero_rest & (1 << h);
        K[h] = StageHalf{x.v, x.r, x.acc, x.w, x.ao, x.vs, x.rs, x.as, x.ws, x.os,
                         z ? x.ao + (int64_t)L->n_wf * L->sv : nullptr, z ? x.ao + rows_of(L) : nullptr};
    }
    const dim3 grid(grid_for(vec ? n / 2 : n, 1024), nfld);
    if (vec)
        hipLaunchKernelGGL(k_orbit_stage<true>, grid, dim3(kThreads), 0, S(stream), n, minv, K[0], g0, gc, gs, g_stride, c,
                           s, K[1], a, b, first ? 1 : 0, L->n_p);
    else
        hipLaunchKernelGGL(k_orbit_stage<false>, grid, dim3(kThreads), 0, S(stream), n, minv, K[0], g0, gc, gs, g_stride,
                           c, s, K[1], a, b, first ? 1 : 0, L->n_p);
    NKV_LAUNCHED();
    return NKV_OK;
}

}  // extern "C"
