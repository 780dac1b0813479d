// fixedp.hip — fixed-point forcing on the device: one time step of selective frequency damping
// (SFD, fixedp.f90:124-216) and of time-delayed feedback (TDF, fixedp.f90:2-121), each as ONE
// streaming pass with the residual norm out of the same pass.
//
// The reference's SFD is ~20 separate k_copy / k_cmult / k_add2 / k_sub3 / nop* sweeps plus normvc
// per step (:157-189, about 50 vector reads and writes); fused it is 6 reads and 4 writes per stored
// row (+ the weights on the velocity rows).  TDF shifts its whole orbit history by one slot per step
// (:77-89, O(norbit N)); as a ring it reads and writes one slot: 5 streams over the velocity rows.
#include "nkv_internal.h"

#ifndef NKV_FP_G
#define NKV_FP_G 768  // workgroup cap of the two kernels (<= NKV_MAXB, the partial slots of one column): 3 per
#endif                // CU, what the SFD kernel's 136 VGPRs admit; +1.5-2.7 % over 1024 on both kernels at
                      // N=1e8, 512 level to -1 % (profiles/fixedp_variants.log)
static_assert(NKV_FP_G >= 1 && NKV_FP_G <= NKV_MAXB, "one reduction partial per workgroup");

namespace {

constexpr int kChunk = 2 * kThreads * kStreamUnr;   // doubles per workgroup per round: divides NKV_TILE,
                                                    // so a chunk never straddles two fields

// Field of chunk ci when it lies in the first nf (<= 3) fields of cpf chunks each, else -1.  No
// division: one comparison per candidate field, once per chunk.
__device__ __forceinline__ int field_of_chunk(int64_t ci, int64_t cpf, int nf) {
    if (ci >= (int64_t)nf * cpf) return -1;
    return (int)(ci >= cpf) + (int)(ci >= 2 * cpf);
}

// ------------------------------------------------------------------------------------------
// SFD, istep >= 1 (fixedp.f90:157-189), per stored row (weighted fields and pressure), evaluated in
// the reference's operation order with no contraction:
//   d     = v_old - qbar                          (k_sub3(qa, oldV, oldQ), :160)
//   m     = ((adt d) + (bdt qa)) + (cdt qb)       (:161-169; qa, qb: the two previous d's)
//   qbar' = qbar + (cutoff dt) m                  (:170-171)
//   fc'   = fc + gain (v_old - qbar')             (:174-176: the LAGGED flow v_old, as the reference)
//   r     = v_old - v;  res2 += w r r             (:186-187) on the rows of the first n_vel fields
//   v_old'= v                                     (:189)
// qd receives d (the buffer that held qc: the host rotates the three pointers, :158-159 without the
// copies).  MONITOR (the continuation branch, :178-183): only the residual and v_old <- v.
// Every thread reads and writes only its own rows and all loads of a chunk precede its stores, so
// v_old, qbar and fc are updated in place.  partials[block] is written by every block.
// ------------------------------------------------------------------------------------------
template <bool MONITOR>
__global__ __launch_bounds__(kThreads) void k_sfd_step(const double* __restrict__ v, double* v_old, double* qbar,
                                                       const double* __restrict__ qa, const double* __restrict__ qb,
                                                       double* __restrict__ qd, double* fc,
                                                       const double* __restrict__ w, double adt, double bdt,
                                                       double cdt, double cdtm, double gain, int64_t chunks,
                                                       int64_t cpf, int64_t sv, int n_vel,
                                                       double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double lds4[4];
    double s = 0.0;
    for (int64_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const int64_t r0 = ci * kChunk + 2 * threadIdx.x;
        const int fld = field_of_chunk(ci, cpf, n_vel);
        double2 vn[kStreamUnr], vo[kStreamUnr], wv[kStreamUnr];
        double2 qm[kStreamUnr], a1[kStreamUnr], a2[kStreamUnr], fv[kStreamUnr];
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u) {
            const int64_t i = r0 + u * 2 * kThreads;
            vn[u] = ldq(v + i);
            vo[u] = ld2(v_old + i);
            if (!MONITOR) {
                qm[u] = ld2(qbar + i);
                a1[u] = ldq(qa + i);
                a2[u] = ldq(qb + i);
                fv[u] = ld2(fc + i);
            }
        }
        if (fld >= 0) {
            const int64_t wr = r0 - (int64_t)fld * sv;
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) wv[u] = ld2(w + wr + u * 2 * kThreads);
        }
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u) {
            const int64_t i = r0 + u * 2 * kThreads;
            if (!MONITOR) {
                const double2 d = make_double2(vo[u].x - qm[u].x, vo[u].y - qm[u].y);
                double2 m = make_double2(adt * d.x + bdt * a1[u].x, adt * d.y + bdt * a1[u].y);
                m = make_double2(m.x + cdt * a2[u].x, m.y + cdt * a2[u].y);
                const double2 qn = make_double2(qm[u].x + cdtm * m.x, qm[u].y + cdtm * m.y);
                const double2 fn = make_double2(fv[u].x + gain * (vo[u].x - qn.x), fv[u].y + gain * (vo[u].y - qn.y));
                st2s(qd + i, d);
                st2(qbar + i, qn);
                st2(fc + i, fn);
            }
            if (fld >= 0) {
                const double rx = vo[u].x - vn[u].x, ry = vo[u].y - vn[u].y;
                s = s + (wv[u].x * rx) * rx;
                s = s + (wv[u].y * ry) * ry;
            }
            st2(v_old + i, vn[u]);
        }
    }
    s = block_sum(s, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// TDF forcing step on one ring slot (fixedp.f90:71-96; the slot holds the flow one period ago, the
// reference's uor(:,1)), over the weighted fields only (pressure and time are not touched):
//   first n_vel fields:  r = v - slot;  res2 += w r r;  fc += gain r;  slot <- v     (:71-75, :90)
//   scalar fields:       slot <- v                                                     (:91-96)
// n_vel = 0 stores only (istep <= norbit, :58-67).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_tdf_step(const double* __restrict__ v, double* slot, double* fc,
                                                       const double* __restrict__ w, double gain, int64_t chunks,
                                                       int64_t cpf, int64_t sv, int n_vel,
                                                       double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double lds4[4];
    double s = 0.0;
    for (int64_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const int64_t r0 = ci * kChunk + 2 * threadIdx.x;
        const int fld = field_of_chunk(ci, cpf, n_vel);
        double2 vn[kStreamUnr], so[kStreamUnr], fv[kStreamUnr], wv[kStreamUnr];
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u) vn[u] = ldq(v + r0 + u * 2 * kThreads);
        if (fld >= 0) {
            const int64_t wr = r0 - (int64_t)fld * sv;
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                const int64_t i = r0 + u * 2 * kThreads;
                so[u] = ld2(slot + i);
                fv[u] = ld2(fc + i);
                wv[u] = ld2(w + wr + u * 2 * kThreads);
            }
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                const double rx = vn[u].x - so[u].x, ry = vn[u].y - so[u].y;
                s = s + (wv[u].x * rx) * rx;
                s = s + (wv[u].y * ry) * ry;
                st2(fc + r0 + u * 2 * kThreads, make_double2(fv[u].x + gain * rx, fv[u].y + gain * ry));
            }
        }
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u) st2(slot + r0 + u * 2 * kThreads, vn[u]);
    }
    s = block_sum(s, lds4);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

int check_n_vel(const nkv_layout* L, int n_vel) {
    if (n_vel < 2 || n_vel > 3 || n_vel > L->n_wf)
        return fail(NKV_EINVAL, "n_vel=%d outside 2..3 or above n_wf=%d", n_vel, L->n_wf);
    return NKV_OK;
}

// Workgroups: one per chunk up to the partial slots the workspace guarantees for one column.
inline int grid_of_chunks(int64_t chunks) { return chunks < NKV_FP_G ? (int)chunks : NKV_FP_G; }

}  // namespace

extern "C" {

int nkv_sfd_step(const nkv_layout* L, const double* w, const double* v, double* v_old, double* qbar,
                 const double* qa, const double* qb, double* qd, double* fc, double adt, double bdt, double cdt,
                 double cutoff_dt, double gain, int n_vel, double* res2_dev, void* ws, unsigned flags,
                 void* stream) {
    CHECK(check_layout(L));
    CHECK(check_n_vel(L, n_vel));
    CHECK(check_ptr(w, "w"));
    CHECK(check_ptr(v, "v"));
    CHECK(check_ptr(v_old, "v_old"));
    CHECK(check_ptr(ws, "ws"));
    if (!res2_dev) return fail(NKV_EINVAL, "res2_dev is NULL");
    const bool monitor = (flags & NKV_SFD_MONITOR) != 0;
    if (!monitor) {
        CHECK(check_ptr(qbar, "qbar"));
        CHECK(check_ptr(qa, "qa"));
        CHECK(check_ptr(qb, "qb"));
        CHECK(check_ptr(qd, "qd"));
        CHECK(check_ptr(fc, "fc"));
        if (qd == qa || qd == qb || qd == qbar || qd == fc || qd == v_old || qd == v)
            return fail(NKV_EINVAL, "qd aliases another vector of the step");
    }
    if (v == v_old) return fail(NKV_EINVAL, "v aliases v_old");
    const int64_t chunks = rows_of(L) / kChunk, cpf = L->sv / kChunk;
    const int g = grid_of_chunks(chunks);
    double* part = partials_of(ws);
    hipStream_t st = S(stream);
    if (g > 0) {   // an empty shard launches nothing
        if (monitor)
            hipLaunchKernelGGL(k_sfd_step<true>, dim3(g), dim3(kThreads), 0, st, v, v_old, qbar, qa, qb, qd, fc, w, adt,
                               bdt, cdt, cutoff_dt, gain, chunks, cpf, L->sv, n_vel, part);
        else
            hipLaunchKernelGGL(k_sfd_step<false>, dim3(g), dim3(kThreads), 0, st, v, v_old, qbar, qa, qb, qd, fc, w, adt,
                               bdt, cdt, cutoff_dt, gain, chunks, cpf, L->sv, n_vel, part);
        NKV_LAUNCHED();
    }
    return launch_reduce_cols(1, part, g, res2_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
}

int nkv_tdf_step(const nkv_layout* L, const double* w, const double* v, double* slot, double* fc, double gain,
                 int n_vel, double* res2_dev, void* ws, unsigned flags, void* stream) {
    CHECK(check_layout(L));
    CHECK(check_n_vel(L, n_vel));
    CHECK(check_ptr(w, "w"));
    CHECK(check_ptr(v, "v"));
    CHECK(check_ptr(slot, "slot"));
    CHECK(check_ptr(ws, "ws"));
    if (!res2_dev) return fail(NKV_EINVAL, "res2_dev is NULL");
    const bool store = (flags & NKV_TDF_STORE) != 0;
    if (!store) CHECK(check_ptr(fc, "fc"));
    if (v == slot || (!store && (fc == slot || fc == v))) return fail(NKV_EINVAL, "v, slot and fc must be distinct");
    const int64_t cpf = L->sv / kChunk, chunks = (int64_t)L->n_wf * cpf;
    const int g = grid_of_chunks(chunks);
    double* part = partials_of(ws);
    hipStream_t st = S(stream);
    if (g > 0) {
        hipLaunchKernelGGL(k_tdf_step, dim3(g), dim3(kThreads), 0, st, v, slot, fc, w, gain, chunks, cpf, L->sv,
                           store ? 0 : n_vel, part);
        NKV_LAUNCHED();
    }
    return launch_reduce_cols(1, part, g, res2_dev, nullptr, 0, nullptr, nullptr, 1 << 30, nan_flag_of(ws), st);
}

}  // extern "C"
