// gs.hip — the sharded gather-scatter's device half (host plan and exchange: nekstab_next_amd/gs.py).
//
// Direct-stiffness averaging (Nek5000's dssum + vmult, dsavg) of nf field segments in one pass over
// the groups of coincident GLL points.  A group's entries name their sources in ascending global
// point number: a local point (src >= 0, an index into every segment) or a value another rank sent
// (src < 0: -(1 + rank * stride + pos), the value of segment f at recv[(rank * nf + f) * stride + pos],
// the all-gathered pack buffers in rank order).  The sum runs in entry order from 0.0 and is scaled by
// 1.0 / count without contraction — k_group_average's arithmetic — so the result does not depend on
// how the points are sharded.  Ranks exchange member values, never partial sums.
//
// Both kernels are element-granular gathers: one lane per group (groups ascend with their first local
// member, so neighbouring lanes touch neighbouring lines) and the L2 does the rest.  A group's entries
// are decoded once into registers and reused for all nf segments; 32-bit indices halve the index
// traffic of k_group_average.  Plain vector loads and stores, no atomics: groups are disjoint.
#include "nkv_internal.h"

namespace {

struct GsSegments {
    double* p[NKV_GS_MAX_FIELDS];
};

constexpr int kGsCached = 8;   // entries of a group held in registers (a 3-D corner: 8 elements)

// send[f * stride + i] = q_f[send_idx[i]]: the index is read once for the nf segments.
__global__ __launch_bounds__(kThreads) void k_gs_pack(int nf, GsSegments q, int64_t n_send,
                                                      const int32_t* __restrict__ send_idx, int64_t stride,
                                                      double* __restrict__ send) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_send; i += (int64_t)gridDim.x * kThreads) {
        const int64_t p = send_idx[i];
        for (int f = 0; f < nf; ++f) send[(int64_t)f * stride + i] = q.p[f][p];
    }
}

// An entry decoded for all segments: a local point index (>= 0), or -(1 + offset of segment 0's value
// in recv); segment f's value then sits f * stride further on.
__device__ inline int64_t gs_decode(int32_t s, int nf, int64_t stride) {
    if (s >= 0) return s;
    const int64_t c = -((int64_t)s + 1);
    const int64_t rank = stride > 0 ? c / stride : 0;
    return -(1 + c + rank * (int64_t)(nf - 1) * stride);
}

__device__ inline double gs_load(const double* __restrict__ q, const double* __restrict__ recv, int64_t off,
                                 int64_t fs) {
    return off >= 0 ? q[off] : recv[-(off + 1) + fs];
}

__global__ __launch_bounds__(kThreads) void k_gs_average(int nf, GsSegments q, int64_t n_groups,
                                                         const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ src,
                                                         const double* __restrict__ recv, int64_t stride) {
#pragma clang fp contract(off)
    for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * kThreads) {
        const int32_t a = start[g], b = start[g + 1];
        const int cnt = b - a;
        const double inv = 1.0 / (double)cnt;
        int64_t off[kGsCached];
#pragma unroll
        for (int i = 0; i < kGsCached; ++i) off[i] = i < cnt ? gs_decode(src[a + i], nf, stride) : 0;
        for (int f = 0; f < nf; ++f) {
            double* __restrict__ qf = q.p[f];
            const int64_t fs = (int64_t)f * stride;
            double v[kGsCached];
#pragma unroll
            for (int i = 0; i < kGsCached; ++i)
                v[i] = i < cnt ? gs_load(qf, recv, off[i], fs) : 0.0;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < kGsCached; ++i)
                if (i < cnt) s = s + v[i];
            for (int i = kGsCached; i < cnt; ++i)   // a vertex shared by more elements than the cache holds
                s = s + gs_load(qf, recv, gs_decode(src[a + i], nf, stride), fs);
            const double m = s * inv;
#pragma unroll
            for (int i = 0; i < kGsCached; ++i)
                if (i < cnt && off[i] >= 0) qf[off[i]] = m;
            for (int i = kGsCached; i < cnt; ++i) {
                const int32_t e = src[a + i];
                if (e >= 0) qf[e] = m;
            }
        }
    }
}

int gs_segments(const char* who, int nf, double* const* q, GsSegments* out) {
    if (nf < 1 || nf > NKV_GS_MAX_FIELDS)
        return fail(NKV_EINVAL, "%s: nf=%d outside 1..%d", who, nf, NKV_GS_MAX_FIELDS);
    if (!q) return fail(NKV_EINVAL, "%s: the segment pointer array is NULL", who);
    for (int f = 0; f < nf; ++f) {
        if (!q[f]) return fail(NKV_EINVAL, "%s: segment %d is NULL", who, f);
        out->p[f] = q[f];
    }
    for (int f = nf; f < NKV_GS_MAX_FIELDS; ++f) out->p[f] = nullptr;
    return NKV_OK;
}

}  // namespace

extern "C" {

int nkv_gs_pack(int nf, double* const* q, int64_t n_v, int64_t n_send, const int32_t* send_idx, int64_t stride,
                double* send, void* stream) {
    if (n_send < 0 || n_v < 0 || stride < 0)
        return fail(NKV_EINVAL, "gs_pack: n_v=%lld, n_send=%lld, stride=%lld must be >= 0", (long long)n_v,
                    (long long)n_send, (long long)stride);
    if (n_v > INT32_MAX) return fail(NKV_EINVAL, "gs_pack: n_v=%lld does not fit the 32-bit indices", (long long)n_v);
    if (n_send > n_v || n_send > stride)
        return fail(NKV_EINVAL, "gs_pack: n_send=%lld exceeds n_v=%lld or stride=%lld", (long long)n_send,
                    (long long)n_v, (long long)stride);
    if (n_send == 0) return NKV_OK;
    GsSegments seg;
    CHECK(gs_segments("gs_pack", nf, q, &seg));
    if (!send_idx || !send) return fail(NKV_EINVAL, "gs_pack: send_idx/send is NULL");
    hipLaunchKernelGGL(k_gs_pack, dim3(grid_for(n_send)), dim3(kThreads), 0, S(stream), nf, seg, n_send, send_idx,
                       stride, send);
    NKV_LAUNCHED();
    return NKV_OK;
}

int nkv_gs_average(int nf, double* const* q, int64_t n_v, int64_t n_groups, const int32_t* start, const int32_t* src,
                   const double* recv, int64_t stride, int n_ranks, void* stream) {
    if (n_groups < 0 || n_v < 0 || stride < 0 || n_ranks < 1)
        return fail(NKV_EINVAL, "gs_average: n_v=%lld, n_groups=%lld, stride=%lld must be >= 0 and n_ranks=%d >= 1",
                    (long long)n_v, (long long)n_groups, (long long)stride, n_ranks);
    if (n_v > INT32_MAX)
        return fail(NKV_EINVAL, "gs_average: n_v=%lld does not fit the 32-bit indices", (long long)n_v);
    if (stride * (int64_t)n_ranks > INT32_MAX)
        return fail(NKV_EINVAL, "gs_average: %d ranks x stride=%lld does not fit the 32-bit indices", n_ranks,
                    (long long)stride);
    if (n_groups == 0) return NKV_OK;
    GsSegments seg;
    CHECK(gs_segments("gs_average", nf, q, &seg));
    if (!start || !src) return fail(NKV_EINVAL, "gs_average: start/src is NULL");
    if (stride > 0 && !recv) return fail(NKV_EINVAL, "gs_average: recv is NULL with stride=%lld", (long long)stride);
    hipLaunchKernelGGL(k_gs_average, dim3(grid_for(n_groups)), dim3(kThreads), 0, S(stream), nf, seg, n_groups, start,
                       src, recv, stride);
    NKV_LAUNCHED();
    return NKV_OK;
}

}  // extern "C"
