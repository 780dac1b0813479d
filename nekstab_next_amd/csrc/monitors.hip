// monitors.hip — the per-time-step monitors of a fixed-point run on the device: the lift / drag / torque
// record of nekStab_torque (utils.f90:718-879) and the running statistics of nekStab_avg
// (postproc.f90:524-646).
//
// The reference evaluates the surface forces over the whole volume every step (mappr, three add2s2,
// comp_sij on every element, three shifted coordinate copies, six unused glmin / glmax: about 40
// N-length streams) although the integrand lives on the object's faces.  k_torque_faces runs one
// workgroup per member face: it stages that element's coordinates and velocity in LDS as k_gradm1 does,
// differentiates only at the face's GLL points (k_gradm1's arithmetic, operation for operation),
// interpolates the pressure only to them and writes the face's twelve sums; k_torque_objects adds the
// members of each object in a fixed order.  Cost: O(member faces), independent of N.
//
// The statistics are ten avg1 / avg2 sweeps per step in the reference (:582-594); k_avg_step is one
// streaming pass over every stored row with the cross moments (the reference's commented avg3 lines
// :597-599) out of the velocities it already holds.
#include "nkv_internal.h"

namespace {

constexpr int kFaceThreads = 256;       // 4 waves: a face has at most 100 points (lx1 = 10 in 3-D)
constexpr int kNQ = 12;                 // dgtq(3, 4): pressure force, viscous force, pressure torque, viscous torque
constexpr int kObjThreads = 64 * kNQ;   // second stage: one wave per entry of dgtq

struct TorqueArgs {
    const double *D, *wg, *Ip;        // GLL derivative matrix, GLL weights, lx2 Gauss -> lx1 GLL matrix (lx1 x lx2)
    const double *xm, *ym, *zm, *u;   // coordinates and velocity (component c at u + c u_stride)
    int64_t u_stride;
    const double *pr, *pm1;           // mesh-2 pressure (lx2^ldim per element) or mesh-1 pressure (n_v)
    int lx2;
    const double* visc_f;             // viscosity field (n_v) or NULL: the scalar `visc`
    double visc;
    const int* faces;                 // [nfaces][3]: local element, face 1..6, object 1..nobj
    double x0[3], dp[3], scale;
    double *dgtq, *sij, *na;
};

// ------------------------------------------------------------------------------------------
// One member face per workgroup.  LDS: D (NX^2), the GLL weights (NX), Ip (NX^2 reserved), X, Y, [Z],
// U[LDIM] (one element each), T (12 terms per face point).  Once the geometric factors and the
// gradient are in registers, X holds the element's mesh-2 pressure.
//
// Face numbers are the preprocessor's: 1: s = -1, 2: r = +1, 3: s = +1, 4: r = -1, 5: t = -1, 6: t = +1.
// Face point fp = a + NX b over the two in-face directions in ascending order ((s, t) on an r-face,
// (r, t) on an s-face, (r, s) on a t-face; 2-D: the one in-face direction).
//   nA_k = +-(g[k][dir] w)    g: the cofactors of geometric_factors (x_s x x_t, x_t x x_r, x_r x x_s; 2-D
//                             (ys, -xs), (-yr, xr)), w = wg[a] wg[b] (2-D wg[a]); + on the +1 face, - on the
//                             -1 face: out of an element with a positive Jacobian
//   pm   = sum_c Ip[k][c] (sum_b Ip[j][b] (sum_a Ip[i][a] p(a, b, c)))   (ascending, first term a product)
//          or pm1 at the point;  pm = ((pm + x dpdx) + y dpdy) [+ z dpdz]             utils.f90:766-768
//   s_ij = G_ij + G_ji        G: nkv_gradm1's gradient at the point (comp_sij without its factor: the
//                             diagonal is G_ii + G_ii)
//   dg(k, 1) = pm nA_k;   dg(k, 2) = -nu ((s_k1 nA_1 + s_k2 nA_2) [+ s_k3 nA_3])
//   dg(:, 3) = r x dg(:, 1), dg(:, 4) = r x dg(:, 2), r = x - x0 (2-D: the z component only)
//   dgtq[face][3 l + k] = (sum over the face points in ascending fp, one by one) scale
// ------------------------------------------------------------------------------------------
template <int LDIM, int NX>
__global__ __launch_bounds__(kFaceThreads) void k_torque_faces(const TorqueArgs A) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int nfp = LDIM == 3 ? NX * NX : NX;
    constexpr int NS = LDIM == 3 ? 6 : 3;
    double* D = lds;
    double* Wg = D + NX * NX;
    double* Ip = Wg + NX;
    double* X = Ip + NX * NX;
    double* Y = X + pts;
    double* Z = Y + pts;                   // 3-D only
    double* U = LDIM == 3 ? Z + pts : Z;   // LDIM velocity components
    double* T = U + LDIM * pts;            // [12][nfp]
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    const int el = A.faces[3 * f], fc = A.faces[3 * f + 1];
    const int64_t p0 = (int64_t)el * pts;
    const int lx2 = A.lx2;
    for (int t = tid; t < NX * NX; t += kFaceThreads) D[t] = A.D[t];
    if (tid < NX) Wg[tid] = A.wg[tid];
    if (A.pr)
        for (int t = tid; t < NX * lx2; t += kFaceThreads) Ip[t] = A.Ip[t];
    for (int t = tid; t < pts; t += kFaceThreads) {
        X[t] = A.xm[p0 + t];
        Y[t] = A.ym[p0 + t];
        if (LDIM == 3) Z[t] = A.zm[p0 + t];
#pragma unroll
        for (int c = 0; c < LDIM; ++c) U[c * pts + t] = A.u[c * A.u_stride + p0 + t];
    }
    __syncthreads();

    // this thread's face point (threads past the face compute on point 0 and store nothing)
    const bool owns = tid < nfp;
    const int fp = owns ? tid : 0;
    const int a = fp % NX, b = fp / NX;
    const int dir = fc >= 5 ? 2 : ((fc & 1) ? 1 : 0);
    const bool plus = fc == 2 || fc == 3 || fc == 6;
    const int c0 = plus ? NX - 1 : 0;
    const int i = dir == 0 ? c0 : a;
    const int j = dir == 0 ? a : (dir == 1 ? c0 : b);
    const int k = LDIM == 3 ? (dir == 2 ? c0 : b) : 0;
    const int r = i + NX * j + NX * NX * k;
    const TilePoint<LDIM, NX> q(D, r, pts);
    double gf[3][3], jacmi;
    geometric_factors<LDIM, NX>(q, X, Y, Z, gf, jacmi);
    double G[3][3];
#pragma unroll
    for (int c = 0; c < LDIM; ++c) {
        double ur, us, ut;
        line_sums<LDIM, NX>(q, U + c * pts, ur, us, ut);
#pragma unroll
        for (int d = 0; d < LDIM; ++d) G[c][d] = physical_derivative<LDIM>(gf, jacmi, d, ur, us, ut);
    }
    const double w = LDIM == 3 ? Wg[a] * Wg[b] : Wg[a];
    double nA[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < LDIM; ++d) {
        const double gd = dir == 0 ? gf[d][0] : ((LDIM == 2 || dir == 1) ? gf[d][1] : gf[d][2]);
        const double v = gd * w;
        nA[d] = plus ? v : -v;
    }
    const double x = X[r], y = Y[r], z = LDIM == 3 ? Z[r] : 0.0;
    const double nu = A.visc_f ? A.visc_f[p0 + r] : A.visc;
    double pm = A.pm1 ? A.pm1[p0 + r] : 0.0;

    if (A.pr) {   // uniform: the element's mesh-2 pressure takes X's place
        const int npp = LDIM == 3 ? lx2 * lx2 * lx2 : lx2 * lx2;
        const int64_t q0 = (int64_t)el * npp;
        __syncthreads();   // every lane has read its coordinates
        for (int t = tid; t < npp; t += kFaceThreads) X[t] = A.pr[q0 + t];
        __syncthreads();
        const double *Ii = Ip + i * lx2, *Ij = Ip + j * lx2, *Ik = Ip + k * lx2;
        auto line = [&](int o) {   // sum_a Ip[i][a] p(a, .)
            double s = Ii[0] * X[o];
            for (int m = 1; m < lx2; ++m) s = s + Ii[m] * X[o + m];
            return s;
        };
        auto plane = [&](int o) {   // sum_b Ip[j][b] line(b)
            double s = Ij[0] * line(o);
            for (int m = 1; m < lx2; ++m) s = s + Ij[m] * line(o + m * lx2);
            return s;
        };
        if constexpr (LDIM == 3) {
            pm = Ik[0] * plane(0);
            for (int m = 1; m < lx2; ++m) pm = pm + Ik[m] * plane(m * lx2 * lx2);
        } else {
            pm = plane(0);
        }
    }
    pm = pm + x * A.dp[0];
    pm = pm + y * A.dp[1];
    if constexpr (LDIM == 3) pm = pm + z * A.dp[2];

    // comp_sij's storage order: 2-D (s11, s22, s12), 3-D (s11, s22, s33, s12, s23, s31)
    double s[3][3];
#pragma unroll
    for (int c = 0; c < LDIM; ++c)
#pragma unroll
        for (int d = 0; d < LDIM; ++d) s[c][d] = G[c][d] + G[d][c];
    if (owns) {
        if (A.sij) {
            double* o = A.sij + (int64_t)f * NS * nfp + fp;
            if constexpr (LDIM == 3) {
                o[0] = s[0][0];
                o[nfp] = s[1][1];
                o[2 * nfp] = s[2][2];
                o[3 * nfp] = s[0][1];
                o[4 * nfp] = s[1][2];
                o[5 * nfp] = s[2][0];
            } else {
                o[0] = s[0][0];
                o[nfp] = s[1][1];
                o[2 * nfp] = s[0][1];
            }
        }
        if (A.na) {
#pragma unroll
            for (int d = 0; d < LDIM; ++d) A.na[((int64_t)f * LDIM + d) * nfp + fp] = nA[d];
        }
        double dg[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) dg[c][0] = dg[c][1] = dg[c][2] = dg[c][3] = 0.0;
#pragma unroll
        for (int c = 0; c < LDIM; ++c) {
            dg[c][0] = pm * nA[c];
            double acc = s[c][0] * nA[0];
            acc = acc + s[c][1] * nA[1];
            if constexpr (LDIM == 3) acc = acc + s[c][2] * nA[2];
            dg[c][1] = -nu * acc;
        }
        const double r1 = x - A.x0[0], r2 = y - A.x0[1], r3 = z - A.x0[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            if constexpr (LDIM == 3) {
                dg[0][2 + l] = r2 * dg[2][l] - r3 * dg[1][l];
                dg[1][2 + l] = r3 * dg[0][l] - r1 * dg[2][l];
            }
            dg[2][2 + l] = r1 * dg[1][l] - r2 * dg[0][l];
        }
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int c = 0; c < 3; ++c) T[(3 * l + c) * nfp + fp] = dg[c][l];
    }
    __syncthreads();
    if (tid < kNQ) {
        const double* t = T + tid * nfp;
        double acc = t[0];
        for (int m = 1; m < nfp; ++m) acc = acc + t[m];
        A.dgtq[(int64_t)f * kNQ + tid] = acc * A.scale;
    }
}

// Second stage, one workgroup: wave q owns entry q of dgtq.  For object o = 1..nobj in turn, lane l adds
// the faces m = l, l + 64, ... of the table that belong to o, in ascending m, onto 0.0; the 64 lane sums
// meet in wave_sum's butterfly (xor 32, 16, 8, 4, 2, 1).  out[o][q] gets lane 0's value, out[0][q] the
// object rows added in ascending o onto 0.0 (utils.f90:839-864).  A fixed order: no atomics.
__global__ __launch_bounds__(kObjThreads) void k_torque_objects(const int* __restrict__ faces, int nfaces, int nobj,
                                                                const double* __restrict__ dgtq,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double total = 0.0;
    for (int o = 1; o <= nobj; ++o) {
        double s = 0.0;
        for (int m = lane; m < nfaces; m += 64)
            if (faces[3 * m + 2] == o) s = s + dgtq[(int64_t)m * kNQ + q];
        s = wave_sum(s);
        total = total + s;
        if (lane == 0) out[o * kNQ + q] = s;
    }
    if (lane == 0) out[q] = total;
}

template <int LDIM, int NX>
void launch_torque(int nfaces, const TorqueArgs& A, hipStream_t st) {
    constexpr int pts = tile_pts<LDIM, NX>();
    constexpr int nfp = LDIM == 3 ? NX * NX : NX;
    constexpr size_t lds = sizeof(double) * ((size_t)2 * NX * NX + NX + (size_t)2 * LDIM * pts + (size_t)kNQ * nfp);
    static_assert(sizeof(double) * (2 * 100 + 10 + 6 * 1000 + 12 * 100) <= 65536, "dynamic LDS within 64 KiB at lx1 = 10");
    hipLaunchKernelGGL((k_torque_faces<LDIM, NX>), dim3(nfaces), dim3(kFaceThreads), lds, st, A);
}

// ------------------------------------------------------------------------------------------
// nekStab_avg's update (postproc.f90:581-599), one pass.  A work item is one chunk of rows of every
// weighted field (so the velocities of a point meet in one thread) or one chunk of the pressure:
//   avg = alpha avg + beta v                      avg1, :582-586
//   rms = alpha rms + (beta v) v                  avg2, :590-594
//   uv, vw, wu = alpha m + (beta f) g             avg3, :597-599: (vx, vy), (vy, vz), (vz, vx); NC = 1: uv only
// Only live rows are stored (the padding rows of avg, rms and the cross buffer are never written).
// ------------------------------------------------------------------------------------------
constexpr int kChunk = 2 * kThreads * kStreamUnr;   // divides NKV_TILE: a chunk never straddles two fields

__device__ __forceinline__ void st_live(double* field, int64_t i, int64_t n, double2 v) {
    if (i + 1 < n)
        st2(field + i, v);
    else if (i < n)
        field[i] = v.x;
}

template <bool RMS, int NC>
__global__ __launch_bounds__(kThreads) void k_avg_step(const double* __restrict__ v, double* __restrict__ avg,
                                                       double* __restrict__ rms, double* __restrict__ cr,
                                                       double alpha, double beta, int64_t cpf, int64_t cpp,
                                                       int64_t sv, int64_t n_v, int64_t n_p, int n_wf) {
#pragma clang fp contract(off)
    constexpr int NV = NC == 3 ? 3 : (NC == 1 ? 2 : 0);   // velocity components the cross moments need
    for (int64_t ci = blockIdx.x; ci < cpf + cpp; ci += gridDim.x) {
        const bool pressure = ci >= cpf;
        const int64_t c = pressure ? ci - cpf : ci;
        const int64_t n = pressure ? n_p : n_v;
        if (c * kChunk >= n) continue;   // a chunk of padding rows only
        const int64_t r0 = c * kChunk + 2 * threadIdx.x;
        double2 keep[NV > 0 ? NV : 1][kStreamUnr];
        auto field = [&](int64_t base, double2 (&vn)[kStreamUnr]) {
            double2 a[kStreamUnr], m[kStreamUnr];
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                const int64_t i = base + r0 + u * 2 * kThreads;
                vn[u] = ldq(v + i);
                a[u] = ld2(avg + i);
                if (RMS) m[u] = ld2(rms + i);
            }
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                const int64_t i = r0 + u * 2 * kThreads;
                st_live(avg + base, i, n, make_double2(alpha * a[u].x + beta * vn[u].x, alpha * a[u].y + beta * vn[u].y));
                if (RMS)
                    st_live(rms + base, i, n, make_double2(alpha * m[u].x + (beta * vn[u].x) * vn[u].x,
                                                           alpha * m[u].y + (beta * vn[u].y) * vn[u].y));
            }
        };
        if (pressure) {
            double2 vn[kStreamUnr];
            field((int64_t)n_wf * sv, vn);
            continue;
        }
#pragma unroll
        for (int f = 0; f < NV; ++f) field((int64_t)f * sv, keep[f]);
        for (int f = NV; f < n_wf; ++f) {
            double2 vn[kStreamUnr];
            field((int64_t)f * sv, vn);
        }
        if constexpr (NC > 0) {
#pragma unroll
            for (int mo = 0; mo < NC; ++mo) {
                const int fi = mo, gi = (mo + 1) % 3 < NV ? (mo + 1) % 3 : 0;
                double* mf = cr + (int64_t)mo * sv;
                double2 m[kStreamUnr];
#pragma unroll
                for (int u = 0; u < kStreamUnr; ++u) m[u] = ld2(mf + r0 + u * 2 * kThreads);
#pragma unroll
                for (int u = 0; u < kStreamUnr; ++u) {
                    const double2 ff = keep[fi][u], gg = keep[gi][u];
                    st_live(mf, r0 + u * 2 * kThreads, n,
                            make_double2(alpha * m[u].x + (beta * ff.x) * gg.x, alpha * m[u].y + (beta * ff.y) * gg.y));
                }
            }
        }
    }
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 8 * (uintptr_t)nb && b0 < a0 + 8 * (uintptr_t)na;
}

}  // namespace

extern "C" {

int nkv_torque(const nkv_layout* L, int lx1, int lx2, int ldim, const double* D, const double* wgll,
               const double* Ipm, const double* xm, const double* ym, const double* zm, const double* u,
               int64_t u_stride, const double* pr, const double* pm1, const double* visc_field, double visc,
               const int* faces_host, const int* faces_dev, int nfaces, int nobj, const double* x0,
               const double* dp_mean, double scale, double* dgtq, double* out, double* sij_out, double* na_out,
               void* stream) {
    static const char who[] = "torque";
    CHECK(check_layout(L));
    if (nobj < 1) return fail(NKV_EINVAL, "%s: nobj=%d < 1", who, nobj);
    if (nfaces < 0) return fail(NKV_EINVAL, "%s: nfaces=%d < 0", who, nfaces);
    CHECK(need(out, who, "out"));
    hipStream_t st = S(stream);
    if (L->n_v == 0 || nfaces == 0) {   // an empty shard, or one that owns no member: zeros, no launch
        if (L->n_v == 0 && nfaces > 0)
            return fail(NKV_EINVAL, "%s: %d member faces on a shard without elements", who, nfaces);
        NKV_HIP(hipMemsetAsync(out, 0, sizeof(double) * kNQ * (size_t)(nobj + 1), st));
        return NKV_OK;
    }
    CHECK(check_mesh_args(who, L, lx1, ldim, zm));
    if (u_stride < L->n_v) return fail(NKV_EINVAL, "%s: u_stride=%lld below n_v=%lld", who, (long long)u_stride, (long long)L->n_v);
    if ((pr != nullptr) == (pm1 != nullptr))
        return fail(NKV_EINVAL, "%s: exactly one of the mesh-2 pressure pr and the mesh-1 pressure pm1 must be given", who);
    const int pts = ldim == 3 ? lx1 * lx1 * lx1 : lx1 * lx1;
    const int64_t nel = L->n_v / pts;
    if (pr) {
        if (lx2 < 1 || lx2 > lx1) return fail(NKV_EINVAL, "%s: lx2=%d outside 1..lx1=%d", who, lx2, lx1);
        const int64_t npp = ldim == 3 ? (int64_t)lx2 * lx2 * lx2 : (int64_t)lx2 * lx2;
        if (L->n_p != nel * npp)
            return fail(NKV_EINVAL, "%s: n_p=%lld is not %lld elements of lx2=%d", who, (long long)L->n_p, (long long)nel, lx2);
        CHECK(need(Ipm, who, "Ipm"));
    }
    CHECK(need(D, who, "D"));
    CHECK(need(wgll, who, "wgll"));
    CHECK(need(xm, who, "xm"));
    CHECK(need(ym, who, "ym"));
    CHECK(need(u, who, "u"));
    CHECK(need(faces_host, who, "faces_host"));
    CHECK(need(faces_dev, who, "faces_dev"));
    CHECK(need(x0, who, "x0"));
    CHECK(need(dp_mean, who, "dp_mean"));
    CHECK(need(dgtq, who, "dgtq"));
    for (int m = 0; m < nfaces; ++m) {
        const int e = faces_host[3 * m], fc = faces_host[3 * m + 1], o = faces_host[3 * m + 2];
        if (e < 0 || e >= nel)
            return fail(NKV_EINVAL, "%s: member %d: element %d outside this shard's 0..%lld", who, m, e, (long long)nel - 1);
        if (fc < 1 || fc > 2 * ldim) return fail(NKV_EINVAL, "%s: member %d: face %d outside 1..%d", who, m, fc, 2 * ldim);
        if (o < 1 || o > nobj) return fail(NKV_EINVAL, "%s: member %d: object %d outside 1..%d", who, m, o, nobj);
    }
    TorqueArgs A;
    A.D = D, A.wg = wgll, A.Ip = Ipm;
    A.xm = xm, A.ym = ym, A.zm = zm, A.u = u, A.u_stride = u_stride;
    A.pr = pr, A.pm1 = pm1, A.lx2 = pr ? lx2 : 1;
    A.visc_f = visc_field, A.visc = visc;
    A.faces = faces_dev;
    for (int d = 0; d < 3; ++d) A.x0[d] = x0[d], A.dp[d] = dp_mean[d];
    A.scale = scale;
    A.dgtq = dgtq, A.sij = sij_out, A.na = na_out;
#define NKV_MON_TORQUE(NX)                                    \
    case NX:                                                  \
        if (ldim == 3) launch_torque<3, NX>(nfaces, A, st);   \
        else launch_torque<2, NX>(nfaces, A, st);             \
        break;
    switch (lx1) { NKV_PP_CASES(NKV_MON_TORQUE) }
#undef NKV_MON_TORQUE
    NKV_LAUNCHED();
    hipLaunchKernelGGL(k_torque_objects, dim3(1), dim3(kObjThreads), 0, st, faces_dev, nfaces, nobj, dgtq, out);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_avg_step(const nkv_layout* L, const double* v, double* avg, double* rms, double* cross, int ncross,
                 double alpha, double beta, void* stream) {
    static const char who[] = "avg_step";
    CHECK(check_layout(L));
    CHECK(check_ptr(v, "v"));
    CHECK(check_ptr(avg, "avg"));
    if (rms) CHECK(check_ptr(rms, "rms"));
    if (cross) {
        CHECK(check_ptr(cross, "cross"));
        if (!rms) return fail(NKV_EINVAL, "%s: the cross moments belong to the ifstatis block: rms is NULL", who);
        if (ncross != 1 && ncross != 3) return fail(NKV_EINVAL, "%s: ncross=%d must be 1 (uv) or 3 (uv, vw, wu)", who, ncross);
        if (L->n_wf < (ncross == 3 ? 3 : 2))
            return fail(NKV_EINVAL, "%s: ncross=%d needs %d velocity fields, n_wf=%d", who, ncross, ncross == 3 ? 3 : 2, L->n_wf);
    }
    const int64_t rows = rows_of(L), ncr = cross ? (int64_t)ncross * L->sv : 0;
    if (overlap(v, rows, avg, rows) || (rms && (overlap(v, rows, rms, rows) || overlap(avg, rows, rms, rows))) ||
        (cross && (overlap(v, rows, cross, ncr) || overlap(avg, rows, cross, ncr) || overlap(rms, rows, cross, ncr))))
        return fail(NKV_EINVAL, "%s: v, avg, rms and the cross buffer must not overlap", who);
    const int64_t cpf = L->n_wf > 0 ? L->sv / kChunk : 0, cpp = L->sp / kChunk;
    const int64_t items = cpf + cpp;
    if (items == 0 || (L->n_v == 0 && L->n_p == 0)) return NKV_OK;   // an empty shard launches nothing
    const int g = items < kMaxBlocks ? (int)items : kMaxBlocks;
    hipStream_t st = S(stream);
#define NKV_MON_AVG(R, NC)                                                                                          \
    hipLaunchKernelGGL((k_avg_step<R, NC>), dim3(g), dim3(kThreads), 0, st, v, avg, rms, cross, alpha, beta, cpf, cpp, \
                       L->sv, L->n_v, L->n_p, L->n_wf)
    if (!rms) NKV_MON_AVG(false, 0);
    else if (!cross) NKV_MON_AVG(true, 0);
    else if (ncross == 1) NKV_MON_AVG(true, 1);
    else NKV_MON_AVG(true, 3);
#undef NKV_MON_AVG
    NKV_LAUNCHED();
    return NKV_OK;
}

}  // extern "C"
