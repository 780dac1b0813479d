// forcing.hip — the body-force hooks of core/forcing.f90 on the device: the sponge function with the
// mask of the dot weights (spng_set + mth_stepf, forcing.f90:157-251; activate_sponge, :101-104) and the
// per-time-step force assembly (nekStab_forcing + nekStab_forcing_temp, :2-79), each as ONE streaming pass.
//
// Traffic model of k_body_force (streams of n_v doubles; a NULL term's stream is not read):
//   per velocity field   reads [ff0] + [fc] + [f_re + f_im] + [v (+ ref in DNS mode)], writes ff
//   per scalar field     reads [ff0] + [fc in DNS mode] + [v (+ ref in DNS mode)], writes ff
//   once per chunk       reads fn (shared by every field of the chunk: the fields are an inner loop)
// The fullest 3-D DNS case (fc, harmonic and sponge terms on the userf zero) reads 5 ldim + 1 streams and
// writes ldim; the perturbation-only case (sponge term alone) reads ldim + 1 and writes ldim.  Composed from
// vector sweeps the former is more than 20 n_v-length sweeps.
// k_sponge_fn reads ldim coordinate streams and writes fn (+ the zeros of the masked weights).
#include "nkv_internal.h"

#ifndef NKV_BF_G
#define NKV_BF_G 1024  // workgroup cap of the two kernels: 4 per CU
#endif

namespace {

constexpr int kChunk = 2 * kThreads * kStreamUnr;   // doubles per workgroup per round: divides NKV_TILE,
                                                    // so a chunk never straddles two fields

// The section constants of one dimension (forcing.f90:192-195 and the section widths of :126-132).
struct SpongeDim {
    double xxmin_c, xxmin, xxmax, xxmax_c, wl, wr;
};
struct SpongeArgs {
    const double* x[3];
    SpongeDim d[3];
    int active[3];
    int ldim;
};

// mth_stepf (forcing.f90:239-251)
__device__ __forceinline__ double mth_stepf(double x) {
#pragma clang fp contract(off)
    if (x <= 0.0010) return 0.0;
    if (x <= 0.9990) return 1.0 / (1.0 + exp(1.0 / (x - 1.0) + 1.0 / x));
    return 1.0;
}

// The five branches of spng_set for one coordinate (forcing.f90:211-224).
__device__ __forceinline__ double sponge_branch(double r, const SpongeDim& s) {
#pragma clang fp contract(off)
    if (r <= s.xxmin_c) return 1.0;                               // constant; xmin
    if (r < s.xxmin) return mth_stepf((s.xxmin - r) / s.wl);      // fall; xmin
    if (r <= s.xxmax) return 0.0;                                 // zero
    if (r < s.xxmax_c) return mth_stepf((r - s.xxmax) / s.wr);    // rise
    return 1.0;                                                   // constant
}

// fn over one padded field (sv rows): the live rows follow spng_set, the padding rows are written 0 (the
// coordinates hold n_v points: no coordinate is read at or beyond n_v).  w (may be NULL) is zeroed where
// fn != 0 (activate_sponge, :102-104).
__global__ __launch_bounds__(kThreads) void k_sponge_fn(SpongeArgs a, int64_t n_v, int64_t chunks,
                                                        double* __restrict__ fn, double* __restrict__ w) {
#pragma clang fp contract(off)
    for (int64_t ci = blockIdx.x; ci < chunks; ci += gridDim.x) {
        const int64_t r0 = ci * kChunk + 2 * threadIdx.x;
        double2 c[3][kStreamUnr];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                c[d][u] = make_double2(0.0, 0.0);
                if (d < a.ldim && a.active[d]) {
                    const int64_t i = r0 + u * 2 * kThreads;
                    if (i + 1 < n_v) {
                        c[d][u] = ldq(a.x[d] + i);
                    } else if (i < n_v) {
                        c[d][u].x = a.x[d][i];
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u) {
            const int64_t i = r0 + u * 2 * kThreads;
            double2 f = make_double2(0.0, 0.0);                   // rzero(spng_fn), :182
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                if (d < a.ldim && a.active[d]) {
                    const double rx = sponge_branch(c[d][u].x, a.d[d]);
                    const double ry = sponge_branch(c[d][u].y, a.d[d]);
                    f.x = rx > f.x ? rx : f.x;                    // max(spng_fn, rtmp), :225
                    f.y = ry > f.y ? ry : f.y;
                }
            }
            if (i >= n_v) f.x = 0.0;
            if (i + 1 >= n_v) f.y = 0.0;
            st2(fn + i, f);
            if (w) {
                if (f.x != 0.0) w[i] = 0.0;
                if (f.y != 0.0) w[i + 1] = 0.0;
            }
        }
    }
}

struct ForceArgs {
    double* ff;
    const double* ff0;   // may alias ff
    const double* fc;
    const double* f_re;
    const double* f_im;
    const double* fn;
    const double* ref;
    const double* v;
    double c, s, st;
    int64_t n_v, sv, chunks;
    int n_wf, n_vel, imag, pert;
};

// One chunk of rows of every weighted field: fn is read once, then per field all loads precede the
// stores (ff may alias ff0; every thread reads and writes only its own rows).  Rows at or beyond n_v are
// not stored.  The operation order is the source's, left to right, uncontracted:
//   velocity (forcing.f90:14-48):  x = ff0 | 0.0;  x = x + fc;
//       real: x = (x + f_re c) - f_im s   imag: x = (x + f_re s) + f_im c
//       DNS:  x = x + (fn (ref - v)) st   perturbation: x = x - fn v
//   scalar (:64-75):  x = ff0 | 0.0;  DNS: x = x + fc;  x = x + fn (ref - t)   perturbation: x = x - fn t
__global__ __launch_bounds__(kThreads) void k_body_force(ForceArgs a) {
#pragma clang fp contract(off)
    for (int64_t ci = blockIdx.x; ci < a.chunks; ci += gridDim.x) {
        const int64_t r0 = ci * kChunk + 2 * threadIdx.x;
        double2 g[kStreamUnr];
#pragma unroll
        for (int u = 0; u < kStreamUnr; ++u)
            g[u] = a.fn ? ld2(a.fn + r0 + u * 2 * kThreads) : make_double2(0.0, 0.0);
        for (int f = 0; f < a.n_wf; ++f) {
            const bool vel = f < a.n_vel;
            const bool use_fc = a.fc && (vel || !a.pert);
            const bool harm = vel && a.f_re;
            const int64_t b = (int64_t)f * a.sv + r0;
            double2 x[kStreamUnr], fcv[kStreamUnr], re[kStreamUnr], im[kStreamUnr], rf[kStreamUnr], vv[kStreamUnr];
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                const int64_t i = b + u * 2 * kThreads;
                x[u] = a.ff0 ? ld2(a.ff0 + i) : make_double2(0.0, 0.0);
                fcv[u] = re[u] = im[u] = rf[u] = vv[u] = make_double2(0.0, 0.0);
                if (use_fc) fcv[u] = ldq(a.fc + i);
                if (harm) {
                    re[u] = ldq(a.f_re + i);
                    im[u] = ldq(a.f_im + i);
                }
                if (a.fn) {
                    vv[u] = ldq(a.v + i);
                    if (!a.pert) rf[u] = ldq(a.ref + i);
                }
            }
#pragma unroll
            for (int u = 0; u < kStreamUnr; ++u) {
                double2 y = x[u];
                if (use_fc) y = make_double2(y.x + fcv[u].x, y.y + fcv[u].y);
                if (harm) {
                    if (!a.imag) {
                        y = make_double2(y.x + re[u].x * a.c, y.y + re[u].y * a.c);
                        y = make_double2(y.x - im[u].x * a.s, y.y - im[u].y * a.s);
                    } else {
                        y = make_double2(y.x + re[u].x * a.s, y.y + re[u].y * a.s);
                        y = make_double2(y.x + im[u].x * a.c, y.y + im[u].y * a.c);
                    }
                }
                if (a.fn) {
                    if (a.pert) {
                        y = make_double2(y.x - g[u].x * vv[u].x, y.y - g[u].y * vv[u].y);
                    } else if (vel) {
                        const double tx = g[u].x * (rf[u].x - vv[u].x), ty = g[u].y * (rf[u].y - vv[u].y);
                        y = make_double2(y.x + tx * a.st, y.y + ty * a.st);
                    } else {
                        y = make_double2(y.x + g[u].x * (rf[u].x - vv[u].x), y.y + g[u].y * (rf[u].y - vv[u].y));
                    }
                }
                const int64_t p = r0 + u * 2 * kThreads;          // row within the field
                const int64_t i = b + u * 2 * kThreads;
                if (p + 1 < a.n_v) {
                    st2(a.ff + i, y);
                } else if (p < a.n_v) {
                    a.ff[i] = y.x;
                }
            }
        }
    }
}

inline int grid_of_chunks(int64_t chunks) { return chunks < NKV_BF_G ? (int)chunks : NKV_BF_G; }

}  // namespace

extern "C" {

int nkv_sponge_fn(const nkv_layout* L, int ldim, const double* xm, const double* ym, const double* zm,
                  const double* sections, unsigned active, double* fn, double* w, void* stream) {
    CHECK(check_layout(L));
    if (ldim != 2 && ldim != 3) return fail(NKV_EINVAL, "nkv_sponge_fn: ldim=%d must be 2 or 3", ldim);
    if (!sections) return fail(NKV_EINVAL, "nkv_sponge_fn: sections is NULL");
    if (active >> ldim) return fail(NKV_EINVAL, "nkv_sponge_fn: active=0x%x names a dimension >= ldim=%d", active, ldim);
    CHECK(check_ptr(fn, "fn"));
    if (w) CHECK(check_ptr(w, "w"));
    if (w == fn) return fail(NKV_EINVAL, "nkv_sponge_fn: w aliases fn");
    SpongeArgs a;
    const double* xs[3] = {xm, ym, zm};
    static const char* const names[3] = {"xm", "ym", "zm"};
    a.ldim = ldim;
    for (int d = 0; d < 3; ++d) {
        a.x[d] = nullptr;
        a.active[d] = d < ldim && ((active >> d) & 1u);
        a.d[d] = SpongeDim{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (!a.active[d]) continue;
        if (L->n_v > 0) CHECK(check_ptr(xs[d], names[d]));
        a.x[d] = xs[d];
        const double* s = sections + 6 * d;
        a.d[d] = SpongeDim{s[0], s[1], s[2], s[3], s[4], s[5]};
        if (!(a.d[d].xxmax > a.d[d].xxmin))   // "Sponge too wide" (:198-199)
            return fail(NKV_EINVAL, "nkv_sponge_fn: dimension %d: xxmax=%g <= xxmin=%g (sponge too wide)", d,
                        a.d[d].xxmax, a.d[d].xxmin);
    }
    const int64_t chunks = L->sv / kChunk;
    const int g = grid_of_chunks(chunks);
    if (g > 0) {   // an empty shard launches nothing
        hipLaunchKernelGGL(k_sponge_fn, dim3(g), dim3(kThreads), 0, S(stream), a, L->n_v, chunks, fn, w);
        NKV_LAUNCHED();
    }
    return NKV_OK;
}

int nkv_body_force(const nkv_layout* L, double* ff, const double* ff0, const double* fc, const double* f_re,
                   const double* f_im, double c, double s, const double* fn, const double* ref, const double* v,
                   double st, int n_vel, unsigned flags, void* stream) {
    CHECK(check_layout(L));
    if (n_vel < 2 || n_vel > 3 || n_vel > L->n_wf)   // as nkv_sfd_step
        return fail(NKV_EINVAL, "n_vel=%d outside 2..3 or above n_wf=%d", n_vel, L->n_wf);
    CHECK(check_ptr(ff, "ff"));
    const bool pert = (flags & NKV_BF_PERTURBATION) != 0, imag = (flags & NKV_BF_IMAG) != 0;
    if (ff0) CHECK(check_ptr(ff0, "ff0"));
    if (fc) CHECK(check_ptr(fc, "fc"));
    if ((f_re != nullptr) != (f_im != nullptr)) return fail(NKV_EINVAL, "f_re and f_im: both or neither");
    if (f_re) {
        CHECK(check_ptr(f_re, "f_re"));
        CHECK(check_ptr(f_im, "f_im"));
    }
    if (fn) {
        CHECK(check_ptr(fn, "fn"));
        CHECK(check_ptr(v, "v"));
        if (!pert) CHECK(check_ptr(ref, "ref"));
    }
    const void* rd[] = {fc, f_re, f_im, fn, fn ? v : nullptr, (fn && !pert) ? ref : nullptr};
    for (const void* p : rd)
        if (p && p == ff) return fail(NKV_EINVAL, "ff aliases an input other than ff0");
    ForceArgs a;
    a.ff = ff;
    a.ff0 = ff0;
    a.fc = fc;
    a.f_re = f_re;
    a.f_im = f_im;
    a.fn = fn;
    a.ref = ref;
    a.v = v;
    a.c = c;
    a.s = s;
    a.st = st;
    a.n_v = L->n_v;
    a.sv = L->sv;
    a.chunks = (L->n_v + kChunk - 1) / kChunk;   // chunks holding a live row (sv is a multiple of kChunk)
    a.n_wf = L->n_wf;
    a.n_vel = n_vel;
    a.imag = imag;
    a.pert = pert;
    const int g = grid_of_chunks(a.chunks);
    if (g > 0) {   // an empty shard launches nothing
        hipLaunchKernelGGL(k_body_force, dim3(g), dim3(kThreads), 0, S(stream), a);
        NKV_LAUNCHED();
    }
    return NKV_OK;
}

}  // extern "C"
