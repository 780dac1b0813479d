/*
 * nekkrylov.h — C ABI of the MI355X (gfx950) Krylov hot path for nekStab.
 *
 * This is the drop-in boundary.  Everything below takes plain device pointers,
 * sizes and a HIP stream (as `void*`), returns an `int` status, and never
 * synchronises the host except where stated.  The reference interfaces each
 * entry point replaces are cited as `file:line` into nekStab_next
 * (reference @ 2025-02-27); see INTEGRATION.md for the Fortran `bind(C)`
 * interface block a nekStab maintainer would add.
 *
 * ---------------------------------------------------------------------------
 * State-vector layout (one nekStab `krylov_vector` / `real_nek_vector`,
 * core/krylov_subspace.f90:12-17, core/nek_vectors.f90:20-31), fp64 in HBM:
 *
 *   [ wf_0 | wf_1 | ... | wf_{n_wf-1} | pr | time | pad ]
 *     each wf_f is `sv` doubles: n_v live points + zero padding
 *     pr is `sp` doubles: n_p live points + zero padding
 *     time is one double at offset  nkv_time_offset(L) = n_wf*sv + sp
 *
 * Weighted fields are vx, vy, [vz], [t_1 .. t_s] — exactly the fields that
 * enter `glsc3(.., bm1s, .., n)` in k_dot / real_dot
 * (krylov_subspace.f90:40-50, nek_vectors.f90:94-104).  Pressure is stored
 * and is touched by every BLAS-1 op (nopaxpby/nopcmult/..., nek_vectors.f90:
 * 229-362) but never enters a dot.  `time` is the scalar component of the
 * vector (krylov_subspace.f90:16).
 *
 * sv and sp are multiples of NKV_TILE (padding rows are zero and their
 * weight is zero), so every kernel streams whole tiles without masking.
 * A Krylov basis is (k+1) vectors at stride `ld` doubles (ld >= time offset+1,
 * multiple of NKV_TILE): Q[c] = Q + c*ld.
 *
 * The weight vector `w` (bm1s, core/NEKSTAB:86-89; zeroed inside a sponge by
 * core/forcing.f90:101-104) has `sv` doubles, shared by every weighted field.
 *
 * Multi-GPU: each rank holds an element-contiguous shard (same layout, local
 * n_v/n_p).  Every reduction entry point writes the LOCAL partial sum to a
 * device buffer; the caller all-reduces it (RCCL) before the consuming entry
 * point runs on the same stream — the MI355X replacement of the per-field
 * MPI_Allreduce hidden in Nek5000's glsc3.
 * ------------------------------------------------------------------------- */
#ifndef NEKKRYLOV_H
#define NEKKRYLOV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NKV_ABI_VERSION 3   /* 3 (round 6): nkv_layout_init added (refuses nelt != nelv); 2 (round 5): the opt-in
                               deferred-basis DCGS2 entry points removed; rotation limited by kept columns */

/* Rows per tile: fields are padded to a multiple of this many doubles. */
#define NKV_TILE 4096
/* Most basis columns one multi-dot (nkv_block_dot / nkv_block_dot2) takes: its per-column partials
 * live in LDS (64 B per column for the two-vector dot).  The reference's k_dim defaults to 100
 * (main.f90:9); GMRES on the cylinder uses 200 (1cyl.usr:14). */
#define NKV_MAX_COLS 1024
/* Most output columns of one basis rotation (nkv_rotate / nkv_rotate_cols): every output column is
 * held in registers while the k input columns stream past (no k-sized state, so any k up to
 * NKV_MAX_COLS).  A Krylov–Schur restart keeps mstart-1 < k_dim columns; the reference's k_dim is
 * at most 200 (1cyl.usr:14), so 256 covers every restart of k_dim <= 257. */
#define NKV_ROT_MAX_OUT 256

/* Status codes (every entry point). */
#define NKV_OK 0
#define NKV_EINVAL 1 /* bad argument / shape                          */
#define NKV_EHIP 2   /* HIP runtime error (see nkv_last_error)        */
#define NKV_ENAN 3   /* NaN detected in a reduction (k_dot :57 guard)  */
#define NKV_ESHAPE 4 /* layout not padded/aligned as documented above  */
#define NKV_ECALLBACK 5 /* a host callback (operator, all-reduce) of a one-call driver failed */
#define NKV_EBREAKDOWN 6 /* NKV_CHECK_BREAKDOWN: the Krylov space became invariant (nkv_arnoldi_factorization) */

/* Flags. */
#define NKV_TIME 0x1u      /* include the `time` slot (dot: add p.time*q.time; BLAS-1: update it) */
#define NKV_ACCUMULATE 0x2u /* block_update: f <- f - Q h   (default)                             */
#define NKV_OVERWRITE 0x4u  /* block_update: f <- + Q h     (k_matmul, krylov_subspace.f90:163)    */
#define NKV_NORM2 0x8u      /* block_update: also write the local ||f||_W^2 partial               */
#define NKV_TIME_DOT 0x10u  /* block_update_dot / block_update+NORM2: time product in the dot/norm */
#define NKV_X_IS_LAST 0x20u /* block_dot2: x is column j-1 of Q (its two dots come from registers)  */
#define NKV_MGS2 0x40u      /* update_hessenberg / arnoldi_factorization: the reference's MGS2 order */
#define NKV_CHECK_BREAKDOWN 0x80u /* one-call factorisations: check the new H columns on return      */
#define NKV_MGS_ICWY 0x100u /* arnoldi_factorization: both MGS passes in inverse compact WY form (3 reads) */
#define NKV_MGS_LAGGED 0x200u /* arnoldi_factorization: MGS2 coefficients, second pass lagged (2 reads) */
#define NKV_SFD_MONITOR 0x400u /* sfd_step: no filter, no forcing (continuation mode): residual and v_old only */
#define NKV_TDF_STORE 0x800u  /* tdf_step: store v in the slot only (the first period), no forcing        */
#define NKV_BF_IMAG 0x1000u   /* body_force: the imaginary branch of the harmonic term (omega_t < 0)          */
#define NKV_BF_PERTURBATION 0x2000u /* body_force: perturbation mode (jp /= 0): ff - fn v, no fc on scalars  */

typedef struct nkv_layout {
    int64_t n_v;  /* live points per weighted field on this rank (lx1*ly1*lz1*nelv)  */
    int64_t n_p;  /* live pressure points on this rank (lx2*ly2*lz2*nelv; 0: no pr)  */
    int64_t sv;   /* padded stride of one weighted field (multiple of NKV_TILE)     */
    int64_t sp;   /* padded length of the pressure segment (multiple of NKV_TILE)   */
    int64_t ld;   /* stride between basis vectors, doubles (multiple of NKV_TILE)   */
    int32_t n_wf; /* number of weighted fields: 2 or 3 velocities + active scalars  */
    int32_t rank0;/* 1 on the rank that owns the replicated `time` term of a dot    */
} nkv_layout;

/* ---- runtime ---------------------------------------------------------- */
int nkv_abi_version(void);
/* Fill *L for one rank's shard from nekStab's SIZE/TOTAL facts (core/nek_vectors.f90:16-31):
 * ldim (2/3, if3d), lx1, lx2 (pressure points per direction; ignored when !ifpo), nelv and nelt (this
 * rank's velocity and temperature/scalar elements), n_scalars (dotted scalars: ifto + ifpsco(:)),
 * ifpo (pressure stored), rank0 (owns the replicated `time` term).  Pads sv, sp, ld to NKV_TILE.
 * NKV_ESHAPE when n_scalars > 0 and nelt != nelv: k_dot / real_dot dot a scalar over nelt elements
 * with the nelv-element weights bm1s (krylov_subspace.f90:36-44, nek_vectors.f90:88-99, NEKSTAB:86),
 * i.e. past the end of bm1s, so conjugate heat transfer layouts have no reference result and are
 * refused.  NKV_EINVAL on bad parameters. */
int nkv_layout_init(nkv_layout* L, int ldim, int lx1, int lx2, int64_t nelv, int64_t nelt, int n_scalars,
                    int ifpo, int rank0);
const char* nkv_last_error(void);
/* Device properties of the current HIP device (host sync-free). */
int nkv_device_info(int* device, int* cu_count, int64_t* hbm_bytes, char* name, int name_len);
/* Bytes of device scratch the reduction entry points need for up to `max_cols` columns. */
size_t nkv_workspace_bytes(const nkv_layout* L, int max_cols);
/* Reads (with a stream sync) and clears the NaN flag kept in the workspace. */
int nkv_check_status(void* ws, void* stream);

/* ---- BLAS-1 over all stored fields (a5/a6) ----------------------------------------------
 * k_zero/real_zero        krylov_subspace.f90:141-150, nek_vectors.f90:70-78
 * k_copy                  krylov_subspace.f90:152-161
 * k_cmult/real_scal       krylov_subspace.f90:94-104,  nek_vectors.f90:116-125
 * real_axpby (time NOT updated unless NKV_TIME)           nek_vectors.f90:127-139,257-277
 * k_add2/k_sub2 = axpby(1,±1), k_sub3                     krylov_subspace.f90:106-139 */
int nkv_zero(const nkv_layout* L, double* x, unsigned flags, void* stream);
int nkv_copy(const nkv_layout* L, double* dst, const double* src, unsigned flags, void* stream);
int nkv_scal(const nkv_layout* L, double* x, double alpha, unsigned flags, void* stream);
int nkv_axpby(const nkv_layout* L, double* x, double alpha, const double* y, double beta,
              unsigned flags, void* stream);
int nkv_sub3(const nkv_layout* L, double* p, const double* q, const double* r, unsigned flags,
             void* stream);
/* x <- x + sign * (*alpha_dev) * y, the scalar read on the device (MGS step, stream-ordered). */
int nkv_axpy_dev(const nkv_layout* L, double* x, const double* alpha_dev, double sign, const double* y,
                 unsigned flags, void* stream);
/* x <- x / sqrt(*nrm2_dev)   (k_normalize, krylov_subspace.f90:75-92); writes sqrt to beta_dev. */
/* Every stored row is scaled, the time slot included (flags reserved, pass 0); eigensolvers.f90's
 * own normalize (nopcmult, :78-116) keeps time — its host restores the slot. */
int nkv_normalize_dev(const nkv_layout* L, double* x, const double* nrm2_dev, double* beta_dev,
                      unsigned flags, void* stream);

/* ---- weighted inner product (a1-a3) -------------------------------------------------------
 * out_dev[0] = sum_fields sum_i a_i*w_i*b_i (+ a.time*b.time if NKV_TIME and rank0)
 * k_dot krylov_subspace.f90:26-60 (time only when uparam(1)==2.1), real_dot nek_vectors.f90:80-114
 * (time always), inner_product eigensolvers.f90:3-56, glsc3 [Nek5000].  LOCAL partial. */
int nkv_dot(const nkv_layout* L, const double* w, const double* a, const double* b, double* out_dev,
            void* ws, unsigned flags, void* stream);

/* ---- block Gram–Schmidt (a7, update_hessenberg_matrix krylov_decomposition.f90:103-189) ----
 * block_dot:    h_dev[0:j] = Q[:,0:j]^T W f  (LOCAL partials, deterministic 2-stage reduction)
 * block_update: f <- f - Q[:,0:j] h           (NKV_ACCUMULATE, default)
 *               f <- Q[:,0:j] h               (NKV_OVERWRITE: k_matmul / mode reconstruction)
 *               with NKV_NORM2 also nrm2_dev[0] = ||f_new||_W^2 local partial (+ f.time^2 with
 *               NKV_TIME_DOT on rank0; NKV_TIME alone updates the slot, not the norm)
 * arnoldi_finish: q_out = f/beta, beta = sqrt(nrm2_dev[0]); H column k written on the device:
 *               hcol[i] = h1[i] + h2[i] (i<j; h2 may be NULL), hcol[j] = beta (H(k+1,k), :183-186) */
int nkv_block_dot(const nkv_layout* L, const double* w, const double* Q, int j, const double* f,
                  double* h_dev, void* ws, unsigned flags, void* stream);
int nkv_block_update(const nkv_layout* L, const double* w, const double* Q, int j, const double* h_dev,
                     double* f, double* nrm2_dev, void* ws, unsigned flags, void* stream);
/* Fused CGS2 middle pass (one read of Q): f <- f - Q[:,0:j] h, then hout_dev[0:j] = Q^T W f_new
 * (LOCAL partials).  NKV_TIME updates f.time, NKV_TIME_DOT adds the time product to hout (rank0). */
int nkv_block_update_dot(const nkv_layout* L, const double* w, const double* Q, int j, const double* h_dev,
                         double* f, double* hout_dev, void* ws, unsigned flags, void* stream);
int nkv_arnoldi_finish(const nkv_layout* L, const double* f, const double* nrm2_dev, double* q_out,
                       int j, const double* h1_dev, const double* h2_dev, double* hcol_dev,
                       unsigned flags, void* stream);

/* The remaining block entry points SURVEY.md §8(b) names:
 * nkv_combine:          out <- Q[:,0:k] y  (k_matmul krylov_subspace.f90:163-209, mode
 *                       reconstruction eigensolvers.f90:565-585; = nkv_block_update NKV_OVERWRITE)
 * nkv_normalize_store:  q_next <- f / sqrt(*nrm2_dev), *beta_dev = sqrt(*nrm2_dev) (the reduced
 *                       ||f||_W^2; update_hessenberg_matrix's last lines :183-186 with Q(k+1) = f, :81)
 * nkv_mgs2_step:        the reference's whole update_hessenberg_matrix in ITS operation order
 *                       (:155-186: two MGS passes, one weighted dot + axpy per column, H(i,k) =
 *                       alpha1 + alpha2, H(k+1,k) = ||f||, q_out = f/||f||), device-side with no
 *                       host sync.  SINGLE PROCESS: its dots are not all-reduced — a sharded host
 *                       runs nkv_dot + all-reduce + nkv_axpy_dev per column (the mgs2 mode of
 *                       nekstab_next_amd.arnoldi).  hcol_dev: j+1 doubles.  NKV_TIME_DOT adds the
 *                       time products to the dots (uparam(1)==2.1, rank0); f.time follows the axpys. */
int nkv_combine(const nkv_layout* L, const double* Q, int k, const double* y_dev, double* out, unsigned flags,
                void* stream);
int nkv_normalize_store(const nkv_layout* L, const double* f, const double* nrm2_dev, double* q_next,
                        double* beta_dev, unsigned flags, void* stream);
int nkv_mgs2_step(const nkv_layout* L, const double* w, const double* Q, int j, double* f, double* q_out,
                  double* hcol_dev, void* ws, unsigned flags, void* stream);
/* One column of an MGS pass fused with the next one's projection (update_hessenberg_matrix's
 * k_cmult + k_sub2 then k_dot, krylov_decomposition.f90:157-166 / :173-180, in that order):
 *   f <- f - (*alpha_dev) qa                 (NKV_TIME: the time slot too, as k_sub2)
 *   *out_dev = <f_new, qb>_W  LOCAL partial  (qb = NULL: <f_new, f_new>, the closing k_normalize);
 * NKV_TIME_DOT adds the time product (rank0).  One read of f for the pair of operations; the MGS2
 * sequences of nkv_update_hessenberg(NKV_MGS2) and nkv_mgs2_step are built from it. */
int nkv_axpy_dot(const nkv_layout* L, const double* w, double* f, const double* alpha_dev, const double* qa,
                 const double* qb, double* out_dev, void* ws, unsigned flags, void* stream);

/* ---- DCGS2: classical Gram–Schmidt with delayed re-orthogonalisation (two reads of Q per step,
 * ONE all-reduce per step, no separate normalisation pass).  Same replacement target as the CGS2
 * entry points above (update_hessenberg_matrix, krylov_decomposition.f90:103-189); the
 * re-orthogonalisation AND the normalisation of q_j are folded into step j+1, the previous H
 * column corrected on the device.  Step j (m = j-1 final columns; Q column m holds u = beta q_j;
 * f = A u):
 *   nkv_block_dot2(Q, j, x=u, y=f) -> h[0:j] = Q^T W u, h[j:2j] = Q^T W f          (all-reduce 2j)
 *   nkv_dcgs2_coef(m, h, h+j, nrm, H, ldh, coef)   H(m,m-1) = beta, row m corrected, column m = c;
 *                                                  coef = [x | c | rinv, y, (beta r)^2, s | a]
 *   nkv_dcgs2_update(Q, m, coef, u, f, Q col j, NULL) -> column m final, column j = the next u
 * nrm points at beta^2: h + m (= u^T W u, the dot's last entry) -- or NULL at the first step
 * (u normalised, beta = 1), or a separately reduced ||u||_W^2 (nkv_dcgs2_update with a non-NULL
 * nrm2 computes it, fused, from the f it writes: one more all-reduce per step).
 * After the last step (m = mend): nkv_block_dot(Q, m+1, u) -> h, nkv_dcgs2_coef(m, h, NULL, h+m, ...),
 * nkv_block_update(Q, m, h, u), nkv_normalize_dev(u, coef+2m+3).
 * H is column-major with leading dimension ldh (>= m+1) in device memory. */
int nkv_block_dot2(const nkv_layout* L, const double* w, const double* Q, int j, const double* x,
                   const double* y, double* h_dev, void* ws, unsigned flags, void* stream);
int nkv_dcgs2_coef(int m, const double* hq_dev, const double* hw_dev, const double* nrm_prev_dev, double* H_dev,
                   int64_t ldh, double* coef_dev, void* ws, void* stream);
int nkv_dcgs2_update(const nkv_layout* L, const double* w, const double* Q, int m, const double* coef_dev,
                     double* qj, const double* win, double* fout, double* nrm2_dev, void* ws, unsigned flags,
                     void* stream);

/* ---- MGS2 in inverse compact WY form (mode "mgs2-icwy"; Swirydowicz et al. 2020) -----------
 * One modified Gram–Schmidt pass of update_hessenberg_matrix (krylov_decomposition.f90:155-168,
 * repeated at :171-180) over q_0..q_{j-1}: alpha_i = <f_i, q_i>_W with f_i = f - sum_{k<i} alpha_k q_k.
 * In exact arithmetic alpha_i = b_i - sum_{k<i} G(i,k) alpha_k with b = Q^T W f (classical dots) and
 * G(i,k) = <q_k, q_i>_W, whether or not the basis is orthonormal (it is not after the reference's
 * unnormalised noise/load seed, eigensolvers.f90:192-223, or a restart with time in k_dot), so
 * alpha = (I + L)^{-1} b, L the strictly lower part of G: the pass becomes one multi-dot, this
 * O(j^2) solve (one workgroup, no host sync) and one block update — three reads of Q per step for
 * both passes instead of the reference order's per-column stream of f.
 * G: row-major, row i at G + i*ldg (ldg >= j); columns k < i are read.  grow (may be NULL): the
 * row G(j-1, 0:j-1) of the newest column, stored into G first (nkv_block_dot2's first j-1 entries
 * with x = q_{j-1}).  x may alias b.  Step j of the factorisation:
 *   nkv_block_dot2(Q, j, x=q_{j-1}, y=f, NKV_X_IS_LAST) -> h; all-reduce 2j
 *   nkv_mgs_icwy_solve(j, G, ldg, h, h+j, h1)                  (pass-1 coefficients)
 *   nkv_block_update_dot(Q, j, h1, f, h2); all-reduce j      (f -= Q h1; h2 = Q^T W f)
 *   nkv_mgs_icwy_solve(j, G, ldg, NULL, h2, h2)              (pass-2 coefficients)
 *   nkv_block_update(Q, j, h2, f, nrm, NKV_NORM2); all-reduce 1; nkv_arnoldi_finish(f, nrm, ...) */
int nkv_mgs_icwy_solve(int j, double* G, int64_t ldg, const double* grow, const double* b, double* x,
                       void* stream);

/* ---- svds: Golub–Kahan–Lanczos with delayed re-orthogonalisation (f1; LightKrylov svds as called by
 * transient_growth_analysis / resolvent_analysis, linear_stab.f90:112,153).  Two bases U, V, each
 * read twice per step (a two-vector multi-dot and a dual update) instead of three times (CGS2).
 * Step j (1-based; V col j-1 and U col j-2 provisional; C = projections of A V on U, D of A^T U on V):
 *   f = A V[j-1];  j = 1: U[0] = f;  else
 *     nkv_block_dot2(U, j-1, x=U[j-2], y=f, NKV_X_IS_LAST) -> h (all-reduce 2(j-1))
 *     nkv_gkl_coef(0, j-2, h, h+(j-1), C, ...)  ->  coef;  C column j-3... finalised
 *     nkv_dcgs2_update(U, j-2, coef, U[j-2], f, U[j-1], NULL)
 *   f = A^T U[j-1];
 *     nkv_block_dot2(V, j, x=V[j-1], y=f, NKV_X_IS_LAST) -> h (all-reduce 2j)
 *     nkv_gkl_coef(1, j-1, h, h+j, D, ...);  nkv_dcgs2_update(V, j-1, coef, V[j-1], f, V[j], NULL)
 * After step k each basis closes its provisional column: nkv_block_dot(Q, m+1, Q[m]) -> h,
 * nkv_gkl_coef(side, m, h, NULL, ...), nkv_block_update(Q, m, coef+2m+5, Q[m]), nkv_normalize_dev(Q[m],
 * coef+2m+3) with m = k-1 (U) and k (V).  Then A V_k = U_k C (k x k upper triangular) and
 * A^T U_k = V_{k+1} D, both bases W-orthonormal.  The coefficient algebra (one workgroup):
 *   a = hq[0:m], r = sqrt(hq[m] - a.a); with hw: M column p+1 (p = m - side) = [hw[0:m] ;
 *   (hw[m] - a.hw[0:m])/r] (raw), coef = [hw[0:m]/r | . | 1/r, M(m,p+1)/r, r^2, 1 | a]; M column p
 *   finalised (p >= 0): M[0:m,p] = (M[0:m,p] - M[0:m,0:p] A_other[:,p] + rho a)/r_other[p],
 *   M[m,p] = rho r / r_other[p], rho = r_self[m-1] (1 at m = 0); A_self[:,m] = a, r_self[m] = r.
 * M, A_self, A_other: device, column-major (ldm, lda >= m+1); r^2 <= 0 raises the NaN flag. */
int nkv_gkl_coef(int side, int m, const double* hq_dev, const double* hw_dev, double* M_dev, int64_t ldm,
                 double* A_self, double* r_self, const double* A_other, const double* r_other, int64_t lda,
                 double* coef_dev, void* ws, void* stream);

/* ---- the whole factorisation natively (a8: arnoldi_factorization, krylov_decomposition.f90:2-99 —
 * the loop :68-96 calling matvec then update_hessenberg_matrix) as ONE call: the DCGS2 sequence
 * above for mstep = mstart..mend, then the closing re-orthogonalisation, orchestrated in C++ (the
 * same entry points in the same order as nekstab_next_amd/arnoldi.py, so the results are identical
 * bit for bit).  For a Fortran/C host that replaces `call arnoldi_factorization(Q, H, mstart, mend,
 * ksize)` without a Python layer.
 *   On entry columns 0..mstart-1 of Q are final and W-orthonormal (column mstart-1: the normalised
 *   seed, or Q(k+1) moved to Q(mstart) by a Krylov–Schur restart) and H columns 0..mstart-2 hold the
 *   factorisation so far (row mstart-1 the restart row).  On return Q columns 0..mend and H columns
 *   0..mend-1 form an Arnoldi factorisation A Q_mend = Q_{mend+1} H.
 *   H_dev: device, column-major, leading dimension ldh >= mend+1.  f: one device vector (scratch).
 *   scratch_dev: nkv_arnoldi_scratch_doubles(mend) doubles of device memory; ws: at least
 *   nkv_workspace_bytes(L, mend + 1) bytes (the multi-dots' partials for up to mend+1 columns).
 *   matvec(mv_user, x, y, stream): y = A x for device vectors x, y, enqueued on `stream`; returns 0.
 *   allreduce(ar_user, buf, n, stream): in-place SUM of n device doubles over the ranks, ordered on
 *   `stream` (ncclAllReduce on it, or a stream sync + MPI_Allreduce); NULL on a single rank.
 *   flags: NKV_TIME_DOT includes the time products in the dots (uparam(1)==2.1, k_dot :52-54);
 *   NKV_CHECK_BREAKDOWN: see "Breakdown" under nkv_arnoldi_factorization below.
 *   A callback's non-zero return stops the factorisation with NKV_ECALLBACK (see nkv_last_error). */
typedef int (*nkv_matvec_fn)(void* user, const double* x, double* y, void* stream);
typedef int (*nkv_allreduce_fn)(void* user, double* buf, int n, void* stream);
size_t nkv_arnoldi_scratch_doubles(int m);
int nkv_arnoldi_dcgs2(const nkv_layout* L, const double* w, double* Q, int mstart, int mend, double* H_dev,
                      int64_t ldh, double* f, double* scratch_dev, void* ws, nkv_matvec_fn matvec, void* mv_user,
                      nkv_allreduce_fn allreduce, void* ar_user, unsigned flags, void* stream);

/* ts_gmres's inner loop (a17: newton_krylov.f90:250-276, each column arnoldi_factorization(Q,H,k,k)
 * then lstsq and norm2(e - H y)) as ONE call on a continuous DCGS2 factorisation: per column k the
 * DCGS2 step of nkv_arnoldi_dcgs2 with the norm of the next provisional vector fused into the update
 * (one more all-reduce), the least-squares residual from nkv_givens_column on H(0:k+1, k-1) with
 * H(k, k-1) = that norm (the column's once-projected coefficients: its O(eps) re-orthogonalisation
 * correction arrives with the next column, so the test needs no lag and no extra matvec), stored in
 * res_hist[k-1]; stop when res^2 < tol2 (the reference's beta**2 < tol, or max(tol, 1e-8) for its
 * iffindiff exit) or at kmax.  Then one closing multi-dot finalises H's last row.
 *   On entry Q column 0 = r0 / beta (W-normalised), beta = ||r0||_W.  On return *k_out = k columns,
 *   H_dev (column-major, ldh >= kmax+1) holds the (k+1) x k Hessenberg matrix of A Q_k = Q_{k+1} H;
 *   Q columns 0..k-1 are final (column k is left unfinished: the solution update does not read it).
 *   The host then solves y = lstsq(H, beta e_1) (dgels, lapack_wrapper.f90:248-300, as the reference)
 *   and forms sol += Q_k y (nkv_combine).  res_hist: kmax host doubles.  scratch_dev:
 *   nkv_arnoldi_scratch_doubles(kmax) doubles; ws: nkv_workspace_bytes(L, kmax + 1).  Callbacks and
 *   flags (NKV_TIME_DOT) as nkv_arnoldi_dcgs2. */
int nkv_gmres_dcgs2(const nkv_layout* L, const double* w, double* Q, int kmax, double beta, double tol2,
                    double* H_dev, int64_t ldh, double* f, double* scratch_dev, void* ws, nkv_matvec_fn matvec,
                    void* mv_user, nkv_allreduce_fn allreduce, void* ar_user, double* res_hist, int* k_out,
                    unsigned flags, void* stream);

/* update_hessenberg_matrix(H, f, Q, k) itself as one call (krylov_decomposition.f90:103-189): the
 * fused 3-pass CGS2 sequence of the block Gram–Schmidt section above (block_dot, all-reduce,
 * block_update_dot, all-reduce, block_update + norm, all-reduce, arnoldi_finish) with the
 * all-reduce as the callback of nkv_arnoldi_dcgs2 (NULL on one rank).  f is orthogonalised twice
 * against Q[:,0:j] (W inner product), q_out = f/||f||_W, hcol_dev[0:j+1] = H(1:k+1, k).  j = 0
 * only normalises.  scratch_dev: nkv_arnoldi_scratch_doubles(j) doubles; ws: nkv_workspace_bytes(L, j)
 * bytes at least.  flags: NKV_TIME_DOT
 * (time products in the dots); NKV_MGS2: the reference's own order instead (:155-186, two MGS passes,
 * one dot + all-reduce + axpy per column; 2j+3 scratch doubles, covered by nkv_arnoldi_scratch_doubles(j)).
 * For per-column consumers (GMRES: newton_krylov.f90:252) and
 * checkpointing Arnoldi, where each column must be final when its step returns. */
int nkv_update_hessenberg(const nkv_layout* L, const double* w, const double* Q, int j, double* f, double* q_out,
                          double* hcol_dev, double* scratch_dev, void* ws, nkv_allreduce_fn allreduce, void* ar_user,
                          unsigned flags, void* stream);

/* arnoldi_factorization (krylov_decomposition.f90:2-99) with per-column orthogonalisation: for
 * mstep = mstart..mend, matvec(Q col mstep-1 -> f), then nkv_update_hessenberg(Q, mstep, f,
 * q_out = Q col mstep, hcol = H col mstep-1).  Same arguments as nkv_arnoldi_dcgs2; every column is
 * final when its step ends and columns < mstart are never written.  flags: NKV_TIME_DOT,
 * NKV_MGS2 (the reference's operation order, its dots all-reduced one at a time through the
 * callback: the sharded form of nkv_mgs2_step), NKV_MGS_ICWY (the same two MGS passes in inverse
 * compact WY form, three reads of Q per step — see nkv_mgs_icwy_solve — for the non-orthonormal bases
 * of the reference's default noise seed; the Gram rows of columns 1..mstart-2 are rebuilt first;
 * scratch: nkv_arnoldi_scratch_doubles(mend), which covers its (mend+1)^2 Gram matrix),
 * NKV_MGS_LAGGED (the same MGS2 coefficients with the second pass lagged into the next step's
 * multi-dot: two reads of Q per step, nkv_lagged_coef on the host between the multi-dot and the
 * dual update, so each step synchronises the stream once; the Gram rows of columns 0..mstart-2 are
 * rebuilt first and H columns 0..mend-1 are downloaded, updated on the host and written back; it
 * uses the Arnoldi relation of the columns before mstart, which the reference's restart breaks in
 * the time slot, so not with NKV_TIME_DOT after a restart), NKV_CHECK_BREAKDOWN.
 *
 * Breakdown (both one-call factorisations).  When the operator's Krylov space closes before mend
 * (A restricted to span(Q) is invariant: a rank-deficient operator), each later f is rounding noise.
 * The reference's MGS2 normalises the noise and carries on; the classical forms cannot: DCGS2's
 * norm sqrt(||u||^2 - ||Q^T W u||^2) cancels to a negative (NaN) and CGS2 leaves O(eps/ratio)
 * components in span(Q).  With NKV_CHECK_BREAKDOWN the driver synchronises the stream on return,
 * and returns NKV_EBREAKDOWN (message: the column and its ratio) if the NaN flag is set (it is
 * cleared) or any new column c has a non-finite entry or |H(c+1,c)| < 1e-8 ||H(0:c+2,c)||.  Normal
 * runs sit at ratios >= 0.1.  nkv_arnoldi_dcgs2 has by then rewritten Q column mstart-1 and H row
 * mstart-1 (the delayed re-orthogonalisation of the seed column): the caller restores both from its
 * own copies and redoes the factorisation with nkv_arnoldi_factorization(..., NKV_MGS2, ...), as
 * nekstab_next_amd.krylov_schur does.  H is replicated, so every rank reaches the same ratio test;
 * the NaN flag is per rank, so a sharded host all-reduces its breakdown decision before branching. */
int nkv_arnoldi_factorization(const nkv_layout* L, const double* w, double* Q, int mstart, int mend, double* H_dev,
                              int64_t ldh, double* f, double* scratch_dev, void* ws, nkv_matvec_fn matvec,
                              void* mv_user, nkv_allreduce_fn allreduce, void* ar_user, unsigned flags, void* stream);

/* ---- Krylov–Schur restart (a10, schur_condensation eigensolvers.f90:421-442) --------------
 * In place: Q[:,0:k] <- Q[:,0:k] * V, V k-by-k column-major (leading dim ldv) in device memory.
 * The time slot is not rotated (the reference copies vx..t only, :421-432).  k <= NKV_ROT_MAX_OUT
 * (NKV_ESHAPE beyond). */
int nkv_rotate(const nkv_layout* L, double* Q, int k, const double* V_dev, int ldv, void* stream);

/* Partial restart rotation, in place: Q[:,0:n_out] <- Q[:,0:k] * V[:,0:n_out], 1 <= n_out <= k.
 * Columns n_out..k-1 are left as they were.  schur_condensation only keeps the mstart selected
 * Schur vectors (eigensolvers.f90:416-459: Q(mstart+1..k) are overwritten by the next
 * factorisation before being read), so the restart calls this with n_out = mstart.
 * k <= NKV_MAX_COLS, n_out <= NKV_ROT_MAX_OUT (NKV_ESHAPE beyond). */
int nkv_rotate_cols(const nkv_layout* L, double* Q, int k, const double* V_dev, int ldv, int n_out,
                    void* stream);

/* The kernel nkv_rotate_cols launches for (L, k, ldv, n_out).  Host only: no device work, callable
 * without a GPU.  nkv_rotate_cols decides through this function, so the two never disagree.
 *   path          : NKV_ROT_PATH_FEW (VALU streaming, <= 16 kept columns), _WIDE (f64 MFMA, 16-byte loads, V
 *                   whole in LDS, 32-bit lane offsets: only while (3 ld + 30) * 8 < 2^32), _STREAM (f64 MFMA,
 *                   V whole in LDS, 64-bit offsets) or _CHUNKED (V through LDS in k-chunks)
 *   inst          : that kernel's template parameter: the kept columns (FEW) or its 16-column blocks
 *   wg_threads    : threads per workgroup of the launch
 *   rows_per_tile : rows one workgroup rotates per trip of its persistent loop
 * The status of a bad layout, k, ldv or n_out is nkv_rotate_cols's; a NULL output is NKV_EINVAL. */
#define NKV_ROT_PATH_FEW 1
#define NKV_ROT_PATH_WIDE 2
#define NKV_ROT_PATH_STREAM 3
#define NKV_ROT_PATH_CHUNKED 4
int nkv_rotate_plan(const nkv_layout* L, int k, int ldv, int n_out, int* path, int* inst, int* wg_threads,
                    int* rows_per_tile);

/* The launch shape of a streaming entry point (the Gram–Schmidt family, BLAS-1, nkv_op_diag) for
 * (L, op, j, flags).  Host only: no device work, callable without a GPU.  Every launcher decides through
 * this function and only maps the plan to its launches, so the two never disagree; every size threshold
 * and band formula of the family lives in it (csrc/core.hip).
 *   op    : NKV_STREAM_BLOCK_DOT   nkv_block_dot (nkv_dot is j = 1)             j = columns, 1..NKV_MAX_COLS
 *           NKV_STREAM_BLOCK_UPDATE nkv_block_update, nkv_combine                j = columns, >= 0
 *           NKV_STREAM_UPDATE_DOT  nkv_block_update_dot                          j = columns, 1..NKV_MAX_COLS
 *           NKV_STREAM_BLOCK_DOT2  nkv_block_dot2                                j = columns, 1..NKV_MAX_COLS
 *           NKV_STREAM_DCGS2_UPDATE nkv_dcgs2_update                             j = m, >= 0
 *           NKV_STREAM_AXPY_DOT    nkv_axpy_dot                                  j ignored
 *           NKV_STREAM_BLAS1       nkv_zero/copy/scal/axpby/sub3/axpy_dev        j ignored
 *           NKV_STREAM_OP_DIAG     nkv_op_diag                                   j ignored
 *           NKV_STREAM_FINISH      nkv_normalize_dev/normalize_store/arnoldi_finish (and the closing
 *                                  normalisation of nkv_mgs2_step)               j ignored
 *   flags : only what changes the shape is read: NKV_NORM2 (block update: the fused norm; DCGS2 update:
 *           "nrm2_dev given"), NKV_OVERWRITE (block update), NKV_X_IS_LAST (two-vector dot).
 * The plan:
 *   kernel        : op, or NKV_STREAM_SPLIT for nkv_block_update_dot past 256 columns or 2^29 rows: that call
 *                   runs the plans of NKV_STREAM_BLOCK_UPDATE then NKV_STREAM_BLOCK_DOT (every other field 0)
 *   pairs         : double2 per thread per tile, the kernel's template parameter (fused pass: 1)
 *   nw, cpw       : fused pass k_update_dot<nw, cpw>: waves per workgroup, columns per wave (else 0)
 *   wg_threads, rows_per_tile : threads per workgroup; rows one workgroup handles per trip of its loop
 *   tiles         : the items the grid's loop walks: row tiles of the whole vector (updates, nkv_axpy_dot), row
 *                   tiles of ONE weighted field (the two dots: grid.y or the block's field loop covers the fields),
 *                   chunks of rows_per_tile rows (BLAS-1, finish, op_diag)
 *   grid_x, grid_y: the first launch's grid
 *   launches      : kernel launches ("row bands"; 0: an empty shard's dot launches only its second stage)
 *   band_tiles    : items per launch (launch i walks [i band_tiles, min((i+1) band_tiles, tiles)))
 *   last_grid_x   : grid.x of the last launch (launches between the first and the last use grid_x)
 *   work_loop     : NKV_STREAM_LOOP_TILES: one item per trip.  NKV_STREAM_LOOP_UNITS (DCGS2 update with norm
 *                   only): one row tile of EVERY weighted field per trip, then the pressure tiles one by one
 *   units         : trips of that loop summed over the grid (a workgroup takes a second trip iff units > grid)
 *   fields_per_block : weighted fields one block walks per row tile (two-vector dot; else 1)
 *   partial_slots, partial_cols : reduction partials per column, and columns, that the second stage sums
 *                   (0: no reduction); grid_x * grid_y * partial_cols slots are written at the most and
 *                   must fit nkv_workspace_bytes(L, max_cols) — max_cols >= the columns of the call
 * NKV_FUSE_ROUNDS and NKV_AXD_ROUNDS are 0 in the product build, so NKV_STREAM_UPDATE_DOT and
 * NKV_STREAM_AXPY_DOT always report one launch; the block update, the DCGS2 update without norm and op_diag
 * launch bands once the vector holds two bands of NKV_*_ROUNDS grid-stride rounds.
 * The status of a bad layout or j is the launcher's own; a NULL plan or an unknown op is NKV_EINVAL. */
#define NKV_STREAM_BLOCK_DOT 1
#define NKV_STREAM_BLOCK_UPDATE 2
#define NKV_STREAM_UPDATE_DOT 3
#define NKV_STREAM_BLOCK_DOT2 4
#define NKV_STREAM_DCGS2_UPDATE 5
#define NKV_STREAM_AXPY_DOT 6
#define NKV_STREAM_BLAS1 7
#define NKV_STREAM_OP_DIAG 8
#define NKV_STREAM_FINISH 9
#define NKV_STREAM_SPLIT 10
#define NKV_STREAM_LOOP_TILES 1
#define NKV_STREAM_LOOP_UNITS 2
typedef struct nkv_plan {
    int64_t kernel, pairs, nw, cpw, wg_threads, rows_per_tile, tiles, grid_x, grid_y, launches, band_tiles,
        last_grid_x, work_loop, units, fields_per_block, partial_slots, partial_cols;
} nkv_plan;
int nkv_stream_plan(const nkv_layout* L, int op, int j, unsigned flags, nkv_plan* plan);

/* ---- synthetic operators (the matvec boundary, linear_operators.f90:17-23) ----------------
 * op_diag: y = d .* x over every stored row; y.time = time_scale * x.time.
 * op_rot2: per weighted point i, (u,v) = (wf_0[i], wf_1[i]):
 *          y = [[c_i, -s_i],[s_i, c_i]] (u,v)   (transpose: s -> -s), other weighted fields and
 *          pressure multiplied by d_rest[row] (may be NULL → 0), y.time = 0. */
int nkv_op_diag(const nkv_layout* L, const double* d, const double* x, double* y, double time_scale,
                void* stream);
int nkv_op_rot2(const nkv_layout* L, const double* c, const double* s, const double* d_rest,
                const double* x, double* y, int transpose, void* stream);
/* op_cdiag: complex diagonal y = c x (conj: conj(c) x) on a re/im pair vector (the complex
 * cmplx_nek_vector{re, im} of nek_vectors.f90:33-42 stored as one real vector: in every segment the
 * re half first, then the im half; c = cr + i ci read at the re rows); y.time = 0.  The synthetic
 * resolvent (i omega - L)^-1 of resolvent_analysis (linear_stab.f90:120-163). */
int nkv_op_cdiag(const nkv_layout* L, const double* cr, const double* ci, const double* x, double* y, int conj,
                 void* stream);

/* ---- sensitivity post-processing (sensitivity.f90) ---------------------------------------
 * These entry points and the two seed kernels below work on field segments only (no time slot):
 * on an empty shard (n_v = 0, a rank without elements) they return NKV_OK without reading any
 * pointer, since its segment arrays are empty (NULL).
 *
 * wave_maker's pointwise product (sensitivity.f90:69-71), after biorthogonalize (:63-66):
 *   out[i] = sqrt(sum_c dRe_c[i]^2 + dIm_c[i]^2) * sqrt(sum_c aRe_c[i]^2 + aIm_c[i]^2),
 * c over the first ncomp (2 or 3, <= n_wf) weighted fields — the velocity components — summed in
 * the reference's left-to-right order without contraction.  out: sv doubles (one field segment;
 * padding rows give 0).  The reference's 2-D case adds its uninitialised vz arrays; here ncomp = 2
 * has no vz terms. */
int nkv_wavemaker(const nkv_layout* L, const double* dRe, const double* dIm, const double* aRe, const double* aIm,
                  double* out, int ncomp, void* stream);
/* bf_sensitivity (sensitivity.f90:81-269), the base-flow sensitivity of Marquet et al.:
 * nkv_gradm1: Nek5000's gradm1 (the calls at sensitivity.f90:170-199; navier5.f, with glmapm1 /
 * xyzrst's geometric factors from the GLL coordinates xm, ym, [zm]) of nfld fields (field f: n_v
 * points at u + f*u_stride, Nek point order, lx1^ldim per element, lx1 <= 10) into
 * grad + (f*ldim + d)*g_stride for direction d = x, y, [z]; the geometric factors are formed once
 * for all nfld fields.  D is the lx1 x lx1 GLL derivative matrix (row-major D[i*lx1+m] = l_m'(z_i),
 * device).  Element-local.  zm exactly when ldim = 3.
 * nkv_bf_sensitivity: the pointwise terms (:202-235) and their sums (:258-259) after gradm1 + dsavg:
 * grad = 4*ncomp*ncomp field segments [dRe, dIm, aRe, aIm][u, v, w][x, y, z] (sv doubles each),
 * out = 6*ncomp segments [tr, ti, pr, pi, sr, si][component].  The reference's dwdz-for-dvdz slips
 * (:204, 207, 213, 216) are kept; its 2-D reads of never-set vz arrays are absent. */
int nkv_gradm1(const nkv_layout* L, int lx1, int ldim, const double* D, const double* xm, const double* ym,
               const double* zm, const double* u, int nfld, int64_t u_stride, double* grad, int64_t g_stride,
               void* stream);
int nkv_bf_sensitivity(const nkv_layout* L, const double* dRe, const double* dIm, const double* aRe,
                       const double* aIm, const double* grad, double* out, int ncomp, void* stream);

/* ---- seeds (utils.f90:258-418; the noise seed is the reference's default, main.f90:29) ---------
 * nkv_mth_rand_add: one weighted field q (n_v points, Nek point order) += mth_rand(il, jl, kl, ieg,
 * xl, fc) (utils.f90:408-418), the pointwise part of op_add_noise (fc per velocity component,
 * :321-331) and add_noise_scal (:258-295); xm/ym/zm are this rank's GLL coordinates (n_v each; zm
 * exactly when lz1 > 1), e_first the 0-based global number of its first element (ieg = e_first+e+1).
 * nkv_group_average: q[m] <- mean of q over m's group, for CSR groups of coincident points
 * (start: n_groups+1 offsets, members: point indices; device arrays) — dssum followed by vmult on
 * one rank (:339-340). */
int nkv_mth_rand_add(const nkv_layout* L, int lx1, int ly1, int lz1, int64_t e_first, const double* xm,
                     const double* ym, const double* zm, double fc1, double fc2, double fc3, double* q,
                     void* stream);
int nkv_group_average(int64_t n_groups, const int64_t* start, const int64_t* members, double* q, void* stream);
/* add_symmetric_seed's perturbation (utils.f90:361-406, 3-D): qx = cos(alpha z) sin(2 pi y),
 * qz = -(2 pi)/alpha cos(alpha z) cos(2 pi y), qt = cos(alpha z) cos(2 pi y) on n_v points (qy is
 * left alone, as the reference does); alpha = 2 pi / (zmax - zmin).  The amplitude scaling
 * 1e-6 / (0.5 sum glsc3(q, bm1, q)) is the host's (two dots and a scal). */
int nkv_symmetric_seed(const nkv_layout* L, const double* ym, const double* zm, double alpha, double* qx,
                       double* qz, double* qt, void* stream);

/* ---- sharded gather-scatter (dssum + vmult / dsavg over element shards; host half: gs.py) --------
 * Direct-stiffness averaging of nf field segments (1 <= nf <= NKV_GS_MAX_FIELDS; q: a HOST array of nf
 * device pointers, each to n_v doubles) in one launch, with 32-bit indices (n_v <= INT32_MAX).
 * nkv_gs_pack: send[f*stride + i] = q[f][send_idx[i]] for i < n_send <= stride (send: nf*stride doubles).
 * nkv_gs_average: for CSR groups (start: n_groups+1 offsets into src) every group's entries are summed
 * in entry order from 0.0, scaled by 1.0/count (no contraction: nkv_group_average's arithmetic), and
 * the mean is written to the group's local entries.  An entry src >= 0 is a local point index; src < 0
 * is -(1 + rank*stride + pos): segment f's value at recv[(rank*nf + f)*stride + pos], the n_ranks pack
 * buffers gathered in rank order (n_ranks*stride <= INT32_MAX; recv may be NULL when stride = 0).
 * Entries are in ascending global point number, so the result is bit-identical for any sharding.
 * Both return NKV_OK without touching memory for a zero count. */
#define NKV_GS_MAX_FIELDS 64
int nkv_gs_pack(int nf, double* const* q, int64_t n_v, int64_t n_send, const int32_t* send_idx, int64_t stride,
                double* send, void* stream);
int nkv_gs_average(int nf, double* const* q, int64_t n_v, int64_t n_groups, const int32_t* start, const int32_t* src,
                   const double* recv, int64_t stride, int n_ranks, void* stream);

/* ---- ts_gmres host helper (a17, newton_krylov.f90:250-269) -------------------------------
 * The least-squares residual ||beta e_1 - H(1:k+2, 1:k+1) y|| after one more Hessenberg column, in
 * O(k) host work (Givens rotations; no device work, no stream).  h: H(0:k+1, k) (0-based column k,
 * overwritten with its triangularised form), cs/sn: the k rotations so far (the new one appended at
 * index k), g: k+2 doubles, g[0] = beta before the first column.  The reference solves the whole
 * system with dgels at every column for this number (:255-258); y itself still comes from dgels on
 * the final system.  k < 0 or a NULL array: returns NaN (message in nkv_last_error). */
double nkv_givens_column(int k, double* h, double* cs, double* sn, double* g);

/* ---- "mgs2-lagged" host algebra (a7 for non-orthonormal bases: the noise / load seed's unnormalised
 * Q(1), eigensolvers.f90:192-223; update_hessenberg_matrix's two MGS passes, krylov_decomposition.f90:
 * 155-186) -------------------------------------------------------------------------------------
 * MGS2's coefficients alpha = (I + L)^-1 Q^T W f for ANY basis (L the strictly lower part of the Gram
 * matrix G), with the second pass of a column lagged into the next step's two-vector multi-dot as
 * DCGS2 does: one multi-dot and one nkv_dcgs2_update per step.  Host-only, no device work.  G:
 * row-major (ldg >= c+1), symmetric; H: column-major (ldh >= c+1), both host memory, updated in place.
 * stage 1 (first step of a factorisation, Q[c] final), 0 (Q[c] holds the previous step's first-pass
 * result u; NKV_ENAN when u has no new direction), 2 (closing pass of the last column).  hv: the
 * step's all-reduced multi-dot (stage 0/1: nkv_block_dot2 with x = Q[c], NKV_X_IS_LAST; stage 2:
 * nkv_block_dot of Q[c] against Q[0:c+1]).  coef: 3c+5 doubles in nkv_dcgs2_update's layout
 * (stage 2: coef[0:c] = the second pass's coefficients, for nkv_block_update).  The algebra in full:
 * drivers.hip; nkv_arnoldi_factorization with NKV_MGS_LAGGED runs the whole sequence. */
int nkv_lagged_coef(int c, int stage, const double* hv, double* G, int64_t ldg, double* H, int64_t ldh,
                    double* coef);

/* ---- fixed-point forcing (core/fixedp.f90; dispatched at core/main.f90:156-176) ------------------
 * Both entries are one streaming pass over state vectors in the layout above; `fc` is the forcing
 * (fcx, fcy, [fcz], fct.., fcp) as one such vector.  res2_dev[0] receives the LOCAL partial of
 * sum w r r over the first n_vel (2 or 3, <= n_wf: the velocities) weighted fields, reduced in a
 * fixed order through the workspace partials (a NaN raises the workspace flag); the caller
 * all-reduces it and forms normvc's l2 = sqrt(res2 / volume) (normvc is Nek5000's, :72, :187).  The
 * time slot of every vector is left alone (the reference never sets oldQ%time and friends).  An empty
 * shard (n_v = 0) writes res2 = 0 and nothing else.
 *
 * nkv_sfd_step: SFD for istep >= 1 (fixedp.f90:157-189), per stored row, in this order, uncontracted:
 *     d     = v_old - qbar                         k_sub3(qa, oldV, oldQ)            :160
 *     m     = ((adt d) + (bdt qa)) + (cdt qb)      tempM                             :161-169
 *     qbar' = qbar + cutoff_dt m                   k_cmult(tempM, cutoff*dt), k_add2 :170-171
 *     fc'   = fc + gain (v_old - qbar')            the lagged flow, as the reference :174-176
 *     r     = v_old - v;  res2 += w r r            nopsub2, normvc (velocities only) :186-187
 *     v_old'= v                                    nopcopy                           :189
 *   qa, qb: the previous two d's; qd receives d.  The host rotates the three buffers (qd holds the
 *   reference's qc on entry; after the call qb <- qa, qa <- qd, qd <- the old qb) instead of the
 *   k_copy(qc, qb), k_copy(qb, qa) of :158-159.  (adt, bdt, cdt): Nek5000's setab3 (:157).
 *   v_old, qbar, fc are updated in place; qd may alias none of the other vectors.
 *   NKV_SFD_MONITOR: the continuation branch (uparam(5) <= 0, :178-183): only r, res2 and v_old';
 *   qbar, qa, qb, qd, fc are not read (may be NULL).
 * nkv_tdf_step: one TDF step on one slot of the orbit ring (fixedp.f90:71-96; `slot` holds the flow
 *   one period ago, the reference's uor/vor/wor/tor(:,1), so its O(norbit N) history shift :77-89
 *   becomes one slot read and written):
 *     first n_vel fields:  r = v - slot;  res2 += w r r;  fc += gain r;  slot <- v   :71-75, :90
 *     scalar fields:       slot <- v                                                  :91-96
 *   The pressure segment of slot and fc is not touched.  NKV_TDF_STORE (istep <= norbit, :58-67):
 *   slot <- v on every weighted field, no forcing (fc may be NULL), res2 = 0. */
int nkv_sfd_step(const nkv_layout* L, const double* w, const double* v, double* v_old, double* qbar,
                 const double* qa, const double* qb, double* qd, double* fc, double adt, double bdt, double cdt,
                 double cutoff_dt, double gain, int n_vel, double* res2_dev, void* ws, unsigned flags,
                 void* stream);
int nkv_tdf_step(const nkv_layout* L, const double* w, const double* v, double* slot, double* fc, double gain,
                 int n_vel, double* res2_dev, void* ws, unsigned flags, void* stream);

/* ---- body-force hooks (core/forcing.f90) ---------------------------------------------------------------
 * Both entries are one streaming pass (16-byte accesses, chunks that never straddle a field, all loads of
 * a chunk before its stores), f64 without contraction in the reference's operand order, no reduction and no
 * host synchronisation.  An empty shard (n_v = 0) launches nothing.
 *
 * nkv_sponge_fn: spng_set + mth_stepf (forcing.f90:157-251) and the weight mask of activate_sponge (:101-104).
 *   xm, ym, zm: this rank's GLL coordinates, n_v points each (device; only the active dimensions are read).
 *   sections: 6 doubles per dimension on the HOST, (xxmin_c, xxmin, xxmax, xxmax_c, wl, wr) of :192-195 with the
 *   section widths of :126-132; `active` holds bit d when dimension d has a sponge (wl > 0 or wr > 0, :186).
 *   Per point, for the active dimensions in ascending order,
 *     r = 1                          x <= xxmin_c          (constant)
 *         mth_stepf((xxmin - x)/wl)  x <  xxmin            (fall)
 *         0                          x <= xxmax
 *         mth_stepf((x - xxmax)/wr)  x <  xxmax_c          (rise)
 *         1                          otherwise             (constant)
 *     fn = max(fn, r),   mth_stepf(a) = 0 (a <= 0.001), 1/(1 + exp(1/(a - 1) + 1/a)) (a <= 0.999), 1 otherwise.
 *   fn: one field of sv doubles; its padding rows [n_v, sv) are written 0 (no coordinate is read there).
 *   w (may be NULL): the dot weights, sv doubles; w[i] = 0 wherever fn[i] != 0, in the same pass.
 *   xxmax <= xxmin in an active dimension is refused (the reference prints "Sponge too wide", :198-199).
 * nkv_body_force: nekStab_forcing + nekStab_forcing_temp (forcing.f90:2-79) over the weighted fields of a
 *   state vector ff.  Every term is optional: a NULL pointer's stream is not read.  Left to right,
 *   first n_vel fields (:14-48):
 *     x = ff0 (NULL: the userf zero, 0.0)
 *     x = x + fc                                                              :14-16
 *     f_re, f_im given, c = cos(omega_t), s = sin(omega_t):                   :19-33
 *       x = (x + f_re c) - f_im s         NKV_BF_IMAG:  x = (x + f_re s) + f_im c
 *     fn given:  x = x + (fn (ref - v)) st     NKV_BF_PERTURBATION:  x = x - fn v  (no strength factor)   :35-50
 *   remaining weighted fields, the scalars (:64-75):
 *     x = ff0 | 0.0;   x = x + fc unless NKV_BF_PERTURBATION (:64);
 *     fn given:  x = x + fn (ref - t)          NKV_BF_PERTURBATION:  x = x - fn t   (no strength, no harmonic)
 *   ff0, fc, f_re, f_im, ref, v: vectors in the layout above (ref: the spng_init snapshot, v: the current
 *   flow or perturbation); fn: one field of sv doubles.  Only the n_v live rows of each weighted field of ff
 *   are written: pressure, padding rows and the time slot are left alone.  ff may alias ff0 (accumulate in
 *   place); any other aliasing of ff returns NKV_EINVAL.  n_vel: 2 or 3 and <= n_wf, as nkv_sfd_step.
 *   Streams of n_v doubles: the fullest 3-D DNS case (fc, harmonic, sponge; ff0 NULL) reads 5 ldim + 1 (fn is
 *   read once per chunk of rows for all fields) and writes ldim; the sponge term alone in perturbation mode
 *   reads ldim + 1 and writes ldim. */
int nkv_sponge_fn(const nkv_layout* L, int ldim, const double* xm, const double* ym, const double* zm,
                  const double* sections, unsigned active, double* fn, double* w, void* stream);
int nkv_body_force(const nkv_layout* L, double* ff, const double* ff0, const double* fc, const double* f_re,
                   const double* f_im, double c, double s, const double* fn, const double* ref, const double* v,
                   double st, int n_vel, unsigned flags, void* stream);

/* ---- per-time-step monitors: surface forces and running statistics ---------------------------------------
 * nkv_torque: nekStab_torque's integrals (utils.f90:758-864) over the member faces this shard owns, with
 *   Nek5000's comp_sij, mappr, drgtrq and create_obj restated from their definitions.  The
 *   cost scales with the number of member faces, not with n_v: one workgroup per face stages that
 *   element in LDS, differentiates and interpolates only at the face's GLL points, and a fixed-order
 *   second stage adds the members of every object.  No atomics.
 *   lx1, ldim, D, xm, ym, zm, u, u_stride: as nkv_gradm1 (velocity component c at u + c u_stride).
 *   wgll: the lx1 GLL weights.  faces: nfaces rows of 3 ints (element local to this shard, 0-based;
 *   face 1..6 in the preprocessor's numbering, 1: s=-1, 2: r=+1, 3: s=+1, 4: r=-1, 5: t=-1, 6: t=+1;
 *   object 1..nobj), once on the HOST (checked before any launch) and once on the device.
 *   Pressure: pr (this shard's n_p mesh-2 values, lx2^ldim per element, interpolated to the face points
 *   with Ipm, the lx1 x lx2 row-major matrix from the lx2 Gauss to the lx1 GLL points) or pm1 (a mesh-1
 *   pressure of n_v points); exactly one of them.  Then pm += x dpdx + y dpdy [+ z dpdz] (:766-768).
 *   visc_field (n_v points) or, when NULL, the scalar visc (param(2)).  x0, dp_mean: 3 doubles on the HOST.
 *   Per face point (fp = a + lx1 b over the in-face directions in ascending order), no contraction:
 *     nA_k = +-(cofactor_k w)           the outward normal times the area: glmapm1's cofactors of the face's
 *                                       direction as nkv_gradm1 forms them, w the GLL face weight
 *     s_ij = G_ij + G_ji                G: nkv_gradm1's gradient, bit for bit (no factor 1/2)
 *     dg(k,1) = pm nA_k                 dg(k,2) = -nu ((s_k1 nA_1 + s_k2 nA_2) [+ s_k3 nA_3])
 *     dg(:,3) = r x dg(:,1)             dg(:,4) = r x dg(:,2),  r = x - x0 (2-D: the z component only)
 *   dgtq[face][3 l + k] = (the terms of the face added one by one in ascending fp) scale  (cmult, :811);
 *   out[o][3 l + k], o = 1..nobj: lane m mod 64 adds the object's faces in ascending table row m onto 0.0,
 *   the 64 lane sums meet in a butterfly (xor 32, 16, 8, 4, 2, 1); out[0]: the object rows added in
 *   ascending o onto 0.0 (:839-864).  The caller all-reduces out (12 (nobj + 1) doubles: the reference's
 *   twelve gop calls, :827-838) and, on more than one rank, forms row 0 again from the reduced rows.
 *   sij_out (may be NULL): [face][3 | 6][fp] in comp_sij's order (s11, s22, s12 | s11, s22, s33, s12, s23,
 *   s31); na_out (may be NULL): [face][ldim][fp].  nfaces = 0 or an empty shard: out is zeroed, no launch.
 *   The unused glmin / glmax of :776-781 are not built.
 * nkv_avg_step: nekStab_avg's update (postproc.f90:581-599) as one pass over every stored row of v:
 *     avg = alpha avg + beta v                        avg1 (:582-586)
 *     rms = alpha rms + (beta v) v                    avg2 (:590-594); rms NULL: ifstatis = .false.
 *     uv, vw, wu = alpha m + (beta f) g               avg3 (:597-599, commented out in the reference):
 *                                                     cross NULL or ncross fields of sv doubles, ncross = 1
 *                                                     (uv) or 3 (uv, vw, wu), from the velocities in registers
 *   avg and rms are vectors in the layout above.  Only live rows are written: padding rows and the time
 *   slot are left alone.  v, avg, rms and the cross buffer must not overlap (NKV_EINVAL).
 *   Streams of live rows: 1 read + 2 read-modify-writes per stored row, + 2 per cross moment. */
int nkv_torque(const nkv_layout* L, int lx1, int lx2, int ldim, const double* D, const double* wgll,
               const double* Ipm, const double* xm, const double* ym, const double* zm, const double* u,
               int64_t u_stride, const double* pr, const double* pm1, const double* visc_field, double visc,
               const int* faces_host, const int* faces_dev, int nfaces, int nobj, const double* x0,
               const double* dp_mean, double scale, double* dgtq, double* out, double* sij_out, double* na_out,
               void* stream);
int nkv_avg_step(const nkv_layout* L, const double* v, double* avg, double* rms, double* cross, int ncross,
                 double alpha, double beta, void* stream);

/* ---- eigenmode kinetic-energy budget (stability_energy_budget, postproc.f90:649-872; uparam(1) = 4.1) ----
 * lx1, ldim, D, xm, ym, zm: as nkv_gradm1 (ldim 2 or 3, lx1 <= 10, lx1^ldim points per element divide
 * n_v, zm exactly when ldim = 3).  Every field is n_v points in Nek point order; strides are in doubles
 * and at least n_v.  All arithmetic is f64 without contraction in the reference's operand order.  Each
 * entry is one grid-stride kernel (the two reducing ones followed by the fixed-order second stage of
 * nkv_dot), no host synchronisation, no atomics, 64-bit point offsets, element-local.  A bad argument
 * returns NKV_EINVAL with a message naming it.
 *
 * nkv_pke_production: compute_production for all base components (postproc.f90:801-836) and the glsc2
 *   of its terms (:728-730) in one tiled pass.  Base component c (ubase + c*b_stride) is differentiated in
 *   LDS with nkv_gradm1's arithmetic (no dsavg, :814, :821, :828), then for direction d
 *     P[c][d] = -0.5 (re_c re_d + im_d im_c) dbase_c/dx_d     (diagonal: re_c**2 + im_c**2; :816-832)
 *   with re_c = dRe + c*m_stride, im_c = dIm + c*m_stride, written to prod + (c*ldim + d)*p_stride (the
 *   reference's energy_budget(:, 3c+d+1); prod may be NULL: integrals only), and
 *     integrals_dev[c*ldim + d] = sum_p bm1[p] P[c][d][p]      (bm1: the mass matrix, n_v weights)
 *   as this rank's LOCAL partial sum, reduced in a fixed order through the workspace partials (run-to-run
 *   deterministic; a NaN raises the workspace flag).  Workspace: ldim^2 <= 9 partials per workgroup, i.e.
 *   nkv_workspace_bytes(L, max_cols >= 4); the grid is capped at the NKV_MAXB workgroups that size
 *   holds.  In 2-D the terms with a z factor are absent (the reference reads never-set arrays there).
 *   An empty shard (n_v = 0) writes ldim^2 zeros and reads nothing else.
 * nkv_divm1: the divergence that closes compute_laplacian (postproc.f90:853-872: Lap a = d2x + d2y + d2z,
 *   :865-869) for nvec vector fields at once: component d of vector v at g + (v*ldim + d)*g_stride,
 *     div_v = (dg_vx/dx + dg_vy/dy) [+ dg_vz/dz]   ->   div + v*d_stride,
 *   every partial derivative exactly what nkv_gradm1 writes for that field and direction (the reference
 *   takes a full gradient of each first derivative and keeps one of its three outputs, :865-867).  The
 *   geometric factors are formed once for all nvec.  An empty shard touches nothing.
 * nkv_pke_dissipation: compute_dissipation's pointwise part (postproc.f90:784-796) and its glsc2 (:729),
 *   streaming (16-byte loads when every base and stride allows).  lap: 2*ncomp segments of l_stride, the
 *   Laplacians of the Re components then of the Im components.  Per point
 *     dummy_c = re_c lap_re_c + im_c lap_im_c;   diss = ((0 + dummy_x) + dummy_y) [+ dummy_z]   (:785-794)
 *     diss = (0.5 diss) nu,  nu = param(2)/param(1)                                              (:796)
 *   written to diss (n_v doubles; may be NULL), and integral_dev[0] = sum_p bm1[p] diss[p], local and
 *   reduced as above (one partial per workgroup).  An empty shard writes 0. */
int nkv_pke_production(const nkv_layout* L, int lx1, int ldim, const double* D, const double* xm, const double* ym,
                       const double* zm, const double* ubase, int64_t b_stride, const double* dRe, const double* dIm,
                       int64_t m_stride, const double* bm1, double* prod, int64_t p_stride, double* integrals_dev,
                       void* ws, void* stream);
int nkv_divm1(const nkv_layout* L, int lx1, int ldim, const double* D, const double* xm, const double* ym,
              const double* zm, const double* g, int nvec, int64_t g_stride, double* div, int64_t d_stride,
              void* stream);
int nkv_pke_dissipation(const nkv_layout* L, const double* dRe, const double* dIm, int64_t m_stride,
                        const double* lap, int64_t l_stride, int ncomp, double nu, const double* bm1, double* diss,
                        double* integral_dev, void* ws, void* stream);

/* ---- flow diagnostics: vortex criteria, filter_s0, energy / enstrophy sums -------------------------
 * (vortex_core and its criteria, postproc.f90:2-522; outpost_vort / nekStab_outpost, utils.f90:420-444,
 * 489-536; nekStab_energy / nekStab_enstrophy, utils.f90:647-716.)
 * lx1, ldim, D, xm, ym, zm and the field conventions: as for the energy budget above.  All arithmetic is
 * f64 without contraction in the reference's operand order; tiled element kernels (the tile of nkv_gradm1),
 * no host synchronisation, no atomics, 64-bit point offsets, element-local.  A bad argument returns
 * NKV_EINVAL with a message naming it; an empty shard (n_v = 0) returns NKV_OK and reads no pointer.
 *
 * Criterion codes; a mask holds bit (1u << code) per criterion.  Output slots are numbered in ascending
 * code order over the selected criteria; vorticity takes three slots in 3-D (x, y, z) and one in 2-D. */
enum nkv_vortex_criterion {
    NKV_VC_VORTICITY = 0,  /* curl of the velocity (comp_vort3 before its averaging): (g32-g23, g13-g31, g21-g12) */
    NKV_VC_LAMBDA2 = 1,    /* middle eigenvalue of S^2 + Omega^2 (Nek5000's lambda2), 3-D only, never filtered */
    NKV_VC_Q = 2,          /* compute_q, :148-175 / compute_secondInv :371-400 (2-D form as written, :395-396) */
    NKV_VC_DELTA = 3,      /* compute_delta, :177-210 */
    NKV_VC_SWIRLING = 4,   /* compute_swirling, :212-305: lambda_ci, filtered, then squared (:298-302) */
    NKV_VC_OMEGA = 5,      /* compute_omega_jc, :31-79 */
    NKV_VC_SYMMETRIC = 6,  /* compute_symmetricVec, :106-125 / compute_symmetric :327-344 */
    NKV_VC_ASSYMETRIC = 7, /* compute_assymetricVec, :127-146 / compute_antisymmetric :307-325 (its '+' kept) */
    NKV_VC_LAMBDA_CI = 8,  /* the swirling strength lambda_ci itself: swirling before its square (filtered alike) */
    NKV_VC_COUNT = 9
};
/* nkv_vortex_criteria: one tiled pass over whole elements.  The ldim velocity components (u + c*u_stride)
 *   and the coordinates are staged in LDS, the tensor g[i][j] = du_i/dx_j is formed per point with every
 *   entry exactly what nkv_gradm1 writes for that component and direction, and every criterion in `mask`
 *   is evaluated from it and stored once at out + slot*o_stride.  A criterion that is also in
 *   `filter_mask` goes through filter_s0 (below) in LDS before its store when F (lx1 x lx1, row-major,
 *   device) is given; F = NULL, or a criterion outside filter_mask, stores the raw value.  vorticity and
 *   lambda2 are never filtered (vortex_core calls lambda2 without filter_s0, :8-9).  swirling is squared
 *   after the filter (:298-302), or directly when unfiltered.  grad (may be NULL) receives the ldim^2
 *   tensor entries at grad + (i*ldim + j)*g_stride.  mask = 0 is allowed with grad (out is then unused).
 *   With I, II, III the invariants of g (:346-435) and P1 = -I, Q1 = II, R1 = -III:
 *     q = II;   delta = (R/2)^2 + (Q/3)^3,  Q = Q1 - P1^2/3,  R = R1 + 2 P1^3/27 - P1 Q1/3;
 *     swirling: cubicLambdaCi(P1, Q1, R1) (:437-474) in 3-D, quadLambdaCi(P1, R1) (:476-500) in 2-D;
 *     omega = b / (a + b + 1e-5),  a = (sum ss_ij^2)^2,  b = (sum oo_ij^2)^2  (sums taken directly, i fastest);
 *     assymetric = ((g12+g21)^2 + (g13+g31)^2 + (g23+g32)^2)/4,  symmetric = that + (g11^2+g22^2+g33^2)/2;
 *     lambda2: the middle eigenvalue of A = S^2 + Omega^2 after five cyclic Jacobi sweeps over (0,1), (0,2),
 *       (1,2) (+ - * / sqrt only; the trigonometric closed form loses half the digits at a double
 *       eigenvalue, i.e. in a solid-body rotation).
 *   lambda2 at ldim = 2 and F with lx1 < 3 are refused.  LDS: (2 lx1^2 + 2 ldim nt) doubles, 49,600 bytes at
 *   lx1 = 10 in 3-D (the coordinate tiles double as the filter's scratch).
 * nkv_filter_s0: Nek5000's filter_s0 / filterq with the matrix F on nfld fields (field f at v + f*v_stride,
 *   result at out + f*o_stride; out may equal v with o_stride = v_stride: in place): along r, then s, then t
 *     v'(i,j,k) = sum_m F[i][m] v(m,j,k)     (m ascending, products not contracted).
 *   The same device routine as the fused filter, so a fused filtered output equals the raw output followed
 *   by this entry bit for bit.  3 <= lx1 <= 10.
 * nkv_energy_components: sums_dev[c] = sum_p f_c[p] w[p] f_c[p] for the ncomp <= 3 segments f + c*f_stride
 *   (glsc3(px, bm1s, px), utils.f90:671-673, 708-710; entries ncomp..2 are 0) and, when t and y are given
 *   (both or neither), sums_dev[3] = sum_p t[p] w[p] y[p] (pot, :674; else 0): four doubles, this rank's
 *   LOCAL partial sums reduced in a fixed order through the workspace partials (four per workgroup,
 *   nkv_workspace_bytes(L, max_cols >= 4)); a NaN raises the workspace flag.  16-byte loads when every
 *   base and stride allows.  An empty shard writes four zeros. */
int nkv_vortex_criteria(const nkv_layout* L, int lx1, int ldim, const double* D, const double* F, const double* xm,
                        const double* ym, const double* zm, const double* u, int64_t u_stride, unsigned mask,
                        unsigned filter_mask, double* out, int64_t o_stride, double* grad, int64_t g_stride,
                        void* stream);
int nkv_filter_s0(const nkv_layout* L, int lx1, int ldim, const double* F, const double* v, int64_t v_stride,
                  int nfld, double* out, int64_t o_stride, void* stream);
int nkv_energy_components(const nkv_layout* L, const double* w, const double* f, int64_t f_stride, int ncomp,
                          const double* t, const double* y, double* sums_dev, void* ws, void* stream);

/* ---- spectral-element advection-diffusion of the dotted fields by a frozen base flow ----------------
 * The equation Nek5000 advances for a passive scalar (ifheat, t), applied to every weighted field on its
 * own: the model operator whose matvec is a time integration over the mesh (LightKrylov's abstract_linop /
 * exponential_prop, linear_operators.f90:39-103, whose body in nekStab is a Nek5000 run).  lx1, ldim, D, xm,
 * ym, zm and the field conventions: as for the energy budget above; w: the lx1 GLL weights (device).  All
 * arithmetic is f64 without contraction; no host synchronisation, no atomics, 64-bit point offsets,
 * element-local (an element sub-range gives the bits of the whole).  A bad argument returns NKV_EINVAL with
 * a message naming it; an empty shard (n_v = 0) returns NKV_OK and reads no pointer.
 *
 * nkv_advdiff_rhs: the LOCAL (unassembled) weak-form right-hand side of nfld fields (field f at
 *   u + f*u_stride, result at r + f*r_stride, diffusivity kappa[f]: nfld doubles on the DEVICE) in one tiled
 *   pass.  With g[d][a], jac the geometric factors of nkv_gradm1 (glmapm1 / xyzrst), d_d u the derivative
 *   as nkv_gradm1 forms it, bm1 = jac w_i w_j [w_k] and D_a^T the transposed line sum along r, s, [t]:
 *     forward:  r = -bm1 (U . grad u) + sum_a D_a^T [ sum_d (g[d][a]/jac) (-kappa bm1 d_d u) ]
 *     adjoint:  r =                     sum_a D_a^T [ sum_d (g[d][a]/jac) (-kappa bm1 d_d u - bm1 U_d u) ]
 *   U: the base flow, component d at U + d*U_stride.  The two are transposes of each other as matrices on
 *   the local points.  Gradient and fluxes stay in LDS (lx1^2 + (ldim + 1) nt doubles, 32,800 bytes at
 *   lx1 = 10 in 3-D).  r must not be u.  The operator is L u = minv dsavg(r), minv = mask / dsavg(bm1):
 *   Nek5000's binvm1 dssum(r) written with dsavg, as comp_vort3 does.
 * nkv_advdiff_bm1: bm1[p] = jac w_i w_j [w_k] (Nek5000's bm1, coef.f), the product the right-hand side
 *   forms, n_v doubles.
 * nkv_advdiff_stage: w_f = v_f + c (minv r_f) for nfld fields in one launch (field f at v + f*v_stride,
 *   r + f*r_stride, w + f*w_stride; minv: n_v doubles): one Horner stage of RK4's polynomial
 *   p(dt L) = 1 + dt L (1 + dt L / 2 (1 + dt L / 3 (1 + dt L / 4))).  v = NULL stands for zero: with
 *   c = 1 the two pointwise halves of the projector x -> minv dsavg(bm1 x).  w may be v.  zero_rest != 0
 *   (w a whole state vector: nfld = n_wf, w_stride = sv) also zeroes the n_p pressure rows and the time
 *   slot of w, as nkv_op_rot2 does for time; padding rows are never written.  16-byte accesses when every
 *   base and stride allows, the same bits either way.
 * nkv_advdiff_cstage: one Horner stage of p(dt G), G = L - i omega, on complex fields with a constant
 *   forcing inside: the step of the rotating-frame time-stepper resolvent (resolvent.ResolventOperator).
 *   nekStab's resolvent_op (linear_operators.f90:348-431) integrates the real state under cos / sin forcing
 *   and takes the imaginary part from a quarter-period run; here u = Re[y e^{i omega t}] turns the forcing
 *   into a constant and the coupling of the halves into -i omega y.  L is the layout of the
 *   re/im PAIR vectors (n_v even): n = n_v / 2 points per half, the halves given by separate pointers with
 *   one stride per operand (field f at ptr + f*stride), since in a pair vector the im half starts n doubles
 *   after the re half, which is 16-byte aligned only for even n.  Per point, in this order, no contraction:
 *     g_re = (minv r_re + omega s_im) [+ f_re]      g_im = (minv r_im - omega s_re) [+ f_im]
 *     w_re = v_re + c g_re                          w_im = v_im + c g_im
 *   s: the stage's source vector, r: the averaged right-hand sides of its halves, minv: n doubles.
 *   v = NULL (both halves) stands for zero, f = NULL (both halves) for no forcing.  w may be v; the spans of
 *   w must not meet those of minv, r, s or f, nor each other.  The adjoint stage passes -omega.
 *   zero_rest != 0 (w a whole pair state vector: nfld = n_wf, w_stride = sv, w_im = w_re + n) also zeroes the
 *   n_p pressure rows and the time slot; padding rows are never written.  16-byte accesses when every
 *   pointer and stride allows, the same bits either way. */
int nkv_advdiff_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, const double* U, int64_t U_stride, const double* kappa,
                    const double* u, int nfld, int64_t u_stride, double* r, int64_t r_stride, int adjoint,
                    void* stream);
int nkv_advdiff_bm1(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, double* bm1, void* stream);
int nkv_advdiff_stage(const nkv_layout* L, const double* v, int64_t v_stride, const double* minv, const double* r,
                      int64_t r_stride, double c, double* w, int64_t w_stride, int nfld, int zero_rest,
                      void* stream);
int nkv_advdiff_cstage(const nkv_layout* L, const double* v_re, const double* v_im, int64_t v_stride,
                       const double* minv, const double* r_re, const double* r_im, int64_t r_stride,
                       const double* s_re, const double* s_im, int64_t s_stride, const double* f_re,
                       const double* f_im, int64_t f_stride, double omega, double c, double* w_re, double* w_im,
                       int64_t w_stride, int nfld, int zero_rest, void* stream);

/* ---- pressure-free viscous Burgers flow: its linearisation, its adjoint and the RK4 stage ------------
 * The nonlinear flow nekStab's Newton-then-stability workflow needs on one mesh (fixed point at
 * uparam(1)=2, stability at 3, adjoint at 3.2; newton_linearized_map, matvec.f90:520-571): the velocity
 * advects itself and every scalar; pressure and incompressibility stay Nek5000's.  Conventions, arithmetic
 * and the treatment of bad arguments and empty shards: as for the advection-diffusion entries above.
 *
 * nkv_linconv_rhs: the LOCAL right-hand side of the convection linearised about a base state B of nfld
 *   fields (field f at B + f*B_stride; its first ldim fields are the advecting velocity), for all nfld
 *   fields of u in one tiled pass.  With r_advdiff(u; U) the two forms of nkv_advdiff_rhs:
 *     forward:  r_f = r_advdiff,f(u; U = B_vel)     - bm1 sum_{d<ldim} u_d d_d B_f
 *     adjoint:  r_f = r_advdiff,adj,f(u; U = B_vel) - [f < ldim] bm1 sum_{f'<nfld} u_f' d_f B_f'
 *   d_d B_f as nkv_gradm1 forms it (element-local), from B_f staged in one more LDS tile: grad B is never
 *   written to global memory.  The sums run in ascending index; the advection-diffusion part keeps the
 *   operand order of nkv_advdiff_rhs.  The two are transposes of each other as matrices on the local points,
 *   so minv dsavg(r_adj) is the exact adjoint of minv dsavg(r_fwd) in the bm1 inner product.  LDS:
 *   lx1^2 + (ldim + 2) nt doubles, 40,800 bytes at lx1 = 10 in 3-D.  nfld >= ldim; the span of r must not
 *   meet those of u or B.  The nonlinear right-hand side needs no entry of its own: it is the forward
 *   nkv_advdiff_rhs with U = u (both read-only there).
 * nkv_rk4_stage: one stage of classical RK4 for nfld fields in one launch (field f at ptr + f*stride).  Per
 *   point, in this order:
 *     k = minv r [+ g]      w = v + a k      acc' = (first ? v : acc) + b k
 *   r: the averaged right-hand side of the stage's state, g: a constant forcing (NULL: none), w: the next
 *   stage's state (NULL on the last stage), acc' written to acc_out, which may be acc or v itself; no other
 *   operand may meet w or acc_out.  v = NULL stands for zero (with first != 0, w = NULL and b = 1:
 *   acc_out = k, the generator itself); otherwise v is read when first != 0 or w is given, acc when
 *   first == 0.
 *   zero_rest != 0 (acc_out a whole state vector: nfld = n_wf, ao_stride = sv) also zeroes the n_p pressure
 *   rows and the time slot; padding rows are never written.  16-byte accesses when every base and stride
 *   allows, the same bits either way. */
int nkv_linconv_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                    const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                    const double* u, int nfld, int64_t u_stride, double* r, int64_t r_stride, int adjoint,
                    void* stream);
int nkv_rk4_stage(const nkv_layout* L, const double* v, int64_t v_stride, const double* minv, const double* r,
                  int64_t r_stride, const double* g, int64_t g_stride, double a, double b, int first,
                  const double* acc, int64_t acc_stride, double* w, int64_t w_stride, double* acc_out,
                  int64_t ao_stride, int nfld, int zero_rest, void* stream);

/* ---- time-periodic base flow of the Burgers flow: the orbit, its tangent and the harmonic forcing -----
 * What nekStab's periodic half needs on one mesh: the forced UPO Newton (uparam(1) = 2.2,
 * newton_krylov.f90:77-91,128-131), Floquet direct / adjoint / intracycle growth (3.11 / 3.21 / 3.31,
 * matvec.f90:176-235,414-468) about the stored orbit uor/vor/wor/tor (ifstorebase) or with the nonlinear flow
 * and the perturbation advanced side by side (ifbase = .true.).  Conventions, arithmetic and the treatment of
 * bad arguments and empty shards: as for the advection-diffusion entries above.
 *
 * nkv_burgers_tangent_rhs: replaces the two solver calls of an ifbase = .true. step (the nonlinear and the
 *   linearised convection of one stage).  For a base state B and a perturbation u of nfld fields each, one
 *   tiled pass writes both LOCAL right-hand sides
 *     r_B,f = r_advdiff,f(B; U = B_vel)               the bits of forward nkv_advdiff_rhs with u = U = B
 *     r_u,f = forward nkv_linconv_rhs(u; B)_f         the same bits
 *   Coordinates and geometric factors once per element group; B_f staged once, its derivatives feeding the
 *   self-advection, the diffusion flux of B and the production term.  19 doubles per point move at ldim = 3,
 *   nfld = 4 where the two launches move 29.  LDS as nkv_linconv_rhs (the flux tiles serve B, then u).
 *   nfld >= ldim; the spans of r_B and r_u must not meet each other, u or B.
 * nkv_burgers_backward_rhs: the right-hand side of the backward sweep of a checkpointed adjoint, in which the
 *   adjoint runs backwards through one segment of the orbit while the segment before it is recomputed from
 *   its checkpoint.  For the base state X being advanced, a stored stage state S and the adjoint variable u
 *   of nfld fields each, one tiled pass writes both LOCAL right-hand sides
 *     r_X,f = r_advdiff,f(X; U = X_vel)               the bits of forward nkv_advdiff_rhs with u = U = X
 *     r_u,f = adjoint nkv_linconv_rhs(u; S)_f         the same bits
 *   Coordinates and geometric factors once per element group; the X sweep first, then the sweep over the
 *   fields of S that closes sum_f' u_f' d_d S_f', then the sweep over u.  23 doubles per point move at
 *   ldim = 3, nfld = 4 where the two launches move 29.  LDS as nkv_linconv_rhs.  nfld >= ldim; the spans of
 *   r_X and r_u must not meet each other, X, S or u; X and S are only read and may be one state.
 * nkv_orbit_stage: one RK4 stage of the base flow under the harmonic forcing g(t) = g0 + cos(wt) gc +
 *   sin(wt) gs (nekStab forces through userf; here the three parts are fields and c, s the cos and sin of the
 *   stage's phase, formed by the host) and, when tr is not NULL, of the tangent in the same launch.  Base half,
 *   per point, in this order:
 *     k = minv r [+ g0] [+ c gc] [+ s gs]      w = v + a k      acc' = (first ? v : acc) + b k
 *   each of g0, gc, gs may be NULL (one g_stride).  Tangent half (tv, tr, tacc, tw, tacc_out): nkv_rk4_stage
 *   without g, with the same a, b, first.  NULL conventions and aliasing per half as nkv_rk4_stage: acc_out may
 *   be the acc or the v of its own half, nothing else may meet an output, of either half.  w is the next
 *   stage's state: pointed into an orbit buffer it stores the orbit with no pass of its own.  zero_rest: bit 0
 *   zeroes pressure and time behind acc_out, bit 1 behind tacc_out (each then a whole state vector).  With
 *   gc = gs = NULL and no tangent half: the bits of nkv_rk4_stage. */
int nkv_burgers_tangent_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                            const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                            const double* u, int nfld, int64_t u_stride, double* r_B, int64_t rB_stride, double* r_u,
                            int64_t ru_stride, void* stream);
int nkv_burgers_backward_rhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                             const double* ym, const double* zm, const double* X, int64_t X_stride, const double* S,
                             int64_t S_stride, const double* kappa, const double* u, int nfld, int64_t u_stride,
                             double* r_X, int64_t rX_stride, double* r_u, int64_t ru_stride, void* stream);
int nkv_orbit_stage(const nkv_layout* L, const double* minv, const double* v, int64_t v_stride, const double* r,
                    int64_t r_stride, const double* g0, const double* gc, const double* gs, int64_t g_stride, double c,
                    double s, double a, double b, int first, const double* acc, int64_t acc_stride, double* w,
                    int64_t w_stride, double* acc_out, int64_t ao_stride, const double* tv, int64_t tv_stride,
                    const double* tr, int64_t tr_stride, const double* tacc, int64_t tacc_stride, double* tw,
                    int64_t tw_stride, double* tacc_out, int64_t tao_stride, int nfld, int zero_rest, void* stream);

/* ---- coupled resolvent: the linearised convection of a complex (re/im pair) perturbation ---------------
 * What a harmonically forced integration about a base state B needs per Horner pass (nekStab's resolvent_op,
 * core/linear_operators.f90:309-431, with the production term of the linearised solver): B is real and does
 * not mix the halves of a pair vector.  Conventions, arithmetic and the treatment of bad arguments and empty
 * shards: as for the advection-diffusion entries above.
 *
 * nkv_linconv_crhs: replaces the two nkv_linconv_rhs calls of a pass.  L is the layout of the real fields
 *   (n_v points per half); the halves come as separate pointers with one stride per operand (field f of the
 *   re half at u_re + f*u_stride, of the im half at u_im + f*u_stride; likewise r_re, r_im with r_stride).  In
 *   a pair segment the im half starts n_v doubles behind the re half: 8-byte alignment is all that is asked.
 *     r_re = nkv_linconv_rhs(u_re; B, adjoint)        r_im = nkv_linconv_rhs(u_im; B, adjoint)        the same bits
 *   Coordinates, geometric factors and the advecting velocity once per element group; forward: B_f staged and
 *   differentiated once per field, its derivatives closing the production term of both halves; adjoint: one
 *   sweep over the base fields accumulates sum_f' u_f' d_d B_f' of both halves.  23 doubles per point move at
 *   ldim = 3, nfld = 4 where the two launches move 30 (12 against 16 at ldim = 2, nfld = 2).  LDS as
 *   nkv_linconv_rhs (the field and flux tiles serve the re, then the im half).  nfld >= ldim; no field segment
 *   of r_re or r_im may meet one of the other half, of u_re, u_im or of B (the halves of a pair vector
 *   interleave, so the segments are compared, not the whole spans). */
int nkv_linconv_crhs(const nkv_layout* L, int lx1, int ldim, const double* D, const double* w, const double* xm,
                     const double* ym, const double* zm, const double* B, int64_t B_stride, const double* kappa,
                     const double* u_re, const double* u_im, int nfld, int64_t u_stride, double* r_re, double* r_im,
                     int64_t r_stride, int adjoint, void* stream);

/* ---- the pressure operators of an incompressible flow and the CG of its projection -------------------
 * Nek5000's opdiv / opgradt / cdabdtp (navier1.f) on the P_N - P_{N-2} pair: the pressure lives on lx2 = lx1 - 2
 * Gauss-Legendre points per direction and element, element-discontinuous (nel lx2^ldim values, elements in
 * order, the first direction fastest).  D, w^, I^: the GLL derivative (lx1 x lx1, row-major), the tensor product
 * of the Gauss weights gw (lx2) and of the Lagrange interpolation interp (lx2 x lx1, row-major) from the GLL to
 * the Gauss points; g[d][a]: the cofactors nkv_gradm1 forms.  Conventions, the tiling, the treatment of bad
 * arguments and of empty shards: as for the advection-diffusion entries.  lx1 = 3 .. 10.  No atomics, no
 * contraction; any element sub-range (pointers offset, n_v shortened) gives the bits of the whole.
 *
 * nkv_pressure_div:   out[e,q] = w^_q I^( sum_{d<ldim} sum_a g[d][a] D_a (mult u_d) )[e,q]: the weak divergence
 *   of the ldim fields at u + d*u_stride, each multiplied pointwise by mult (n_v values) when mult is not NULL.
 *   With pv (a pressure-mesh vector) and partials given, workgroup b also writes its share of pv.out, sum out
 *   and sum pv to partials[b], partials[NKV_PRESSURE_PARTIALS + b], partials[2 NKV_PRESSURE_PARTIALS + b]
 *   (b < at most NKV_PRESSURE_PARTIALS workgroups, a fixed count for a given n_v; other slots are not touched).
 * nkv_pressure_gradt: t_d = sum_a D_a^T [ g[d][a] I^^T(w^ p) ], the ldim unassembled GLL fields at
 *   t + d*t_stride: the matrix transpose of nkv_pressure_div.  With res given, p <- first ? res : res + beta p
 *   is formed on the load and stored back, beta = (sum of the B values at rr_new) / (sum of those at rr_old),
 *   0 when the denominator is.
 * nkv_pressure_cg_update: the pointwise third of a CG iteration over n pressure values.  red: the three rows
 *   of Br partials nkv_pressure_div wrote (Br = NKV_PRESSURE_PARTIALS, or 1 after the caller reduced them over
 *   ranks); rr_old: Bo partials of r.r.  mu = closed ? sum Ep * inv_n : 0; alpha = r.r / (p.Ep - mu sum p), 0
 *   when the denominator is;  x <- x + alpha p,  r <- r - alpha (Ep - mu);  workgroup b writes its share of the
 *   new r.r to rr_out[b] (at most NKV_PRESSURE_PARTIALS workgroups).  init: x <- 0, r <- Ep - mu.
 *   Every workgroup sums partials in one fixed order: the same input gives the same bits. */
#define NKV_PRESSURE_PARTIALS 1024
int nkv_pressure_div(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                     const double* xm, const double* ym, const double* zm, const double* u, int64_t u_stride,
                     const double* mult, double* out, const double* pv, double* partials, void* stream);
int nkv_pressure_gradt(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                       const double* xm, const double* ym, const double* zm, double* p, const double* res,
                       const double* rr_new, const double* rr_old, int B, int first, double* t, int64_t t_stride,
                       void* stream);
int nkv_pressure_cg_update(int64_t n, double* x, double* r, const double* p, const double* Ep, const double* red, int Br,
                           const double* rr_old, int Bo, double inv_n, int closed, int init, double* rr_out,
                           void* stream);
int nkv_pressure_partials(void);

/* ---- the same three over two systems: the CG of both halves of a pair vector in one launch each -------
 * A resolvent stage projects the re and the im half of a complex vector: two pressure solves on one mesh.  The
 * systems share the coordinates, the factors, D, interp, gw and mult, which are staged and formed once per
 * element group; the LDS tiles then serve system 0, then system 1 (LDS as the single-system kernels).  The
 * systems come as separate pointers with one stride per operand, as in nkv_linconv_crhs: only 8-byte alignment
 * is asked of either (in a pair vector the im half starts n_v doubles behind the re half, and n_v may be odd).
 * active: bit s = system s, 1..3.  An inactive system is neither read nor written (its pointers may be NULL):
 * not its vectors, nor its outputs, nor its partial rows.  For an active system every output and partial is
 * bit for bit what the single-system entry gives on that system's operands alone: the same arithmetic in the
 * same order, the same grid and the same slot per workgroup, no atomics, no contraction; element sub-ranges
 * give the bits of the whole.  A system named in active with a NULL operand, and written spans that meet each
 * other or a span that is read (strided fields segment by segment), are NKV_EINVAL.  Empty shards as above.
 *
 * nkv_pressure_div2:   out_s = nkv_pressure_div(u_s; mult); with pv_s and partials given (all active systems or
 *   none) the three rows of system s go to partials + s * 3 NKV_PRESSURE_PARTIALS.
 * nkv_pressure_gradt2: t_s = nkv_pressure_gradt(p_s); with res_s given (all active systems or none)
 *   p_s <- first ? res_s : res_s + beta_s p_s, beta_s from the B values at rr_new + s*B over those at
 *   rr_old + s*B.  first is shared.
 * nkv_pressure_cg_update2: nkv_pressure_cg_update on (x_s, r_s, p_s, Ep_s) with the three rows of system s at
 *   red + s * 3 Br, its r.r at rr_old + s*Bo, and its new partials written to rr_out + s * NKV_PRESSURE_PARTIALS:
 *   its own mu and alpha.  inv_n, closed and init are shared. */
int nkv_pressure_div2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                      const double* xm, const double* ym, const double* zm, const double* u0, const double* u1,
                      int64_t u_stride, const double* mult, double* out0, double* out1, const double* pv0,
                      const double* pv1, double* partials, int active, void* stream);
int nkv_pressure_gradt2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                        const double* xm, const double* ym, const double* zm, double* p0, double* p1, const double* res0,
                        const double* res1, const double* rr_new, const double* rr_old, int B, int first, double* t0,
                        double* t1, int64_t t_stride, int active, void* stream);
int nkv_pressure_cg_update2(int64_t n, double* x0, double* x1, double* r0, double* r1, const double* p0, const double* p1,
                            const double* Ep0, const double* Ep1, const double* red, int Br, const double* rr_old, int Bo,
                            double inv_n, int closed, int init, double* rr_out, int active, void* stream);

/* ---- the fast-diagonalisation preconditioner of that CG -------------------------------------------------
 * M = blockdiag(M_e), M_e = (S x .. x S) diag( 1 / sum_d c[e][d] lambda_{i_d} ) (S^T x .. x S^T) on the lx2^ldim
 * pressure values of element e (i_1 along the first, fastest direction): the exact inverse of a separable model of
 * the element's block of E.  S (lx2 x lx2, row-major, S^T B^ S = I) and lambda (lx2) are the generalised eigenpairs
 * of the 1-D reference problem and c (nel x ldim, row-major) the element scales; pressure.py documents and builds
 * them.  Whole elements per workgroup, sum factorisation through LDS; the pressure mesh only, no dsavg, no atomics,
 * no contraction; any element sub-range (r, z, c offset, nel shortened) gives the bits of the whole.  lx1 = 3 .. 10.
 *
 * nkv_pressure_precond:  z = M r over nel elements; z may not meet r.  With partials given workgroup b also writes
 *   its share of r.z to partials[b] and of sum z to partials[NKV_PRESSURE_PARTIALS + b] (a fixed count of at most
 *   NKV_PRESSURE_PARTIALS workgroups for a given nel; other slots are not touched).  nel = 0 touches nothing.
 * nkv_pressure_precond2: the same for two systems (conventions of the two-system entries above: active, the bits
 *   of the single-system entry, overlapping spans refused); r_s.z_s goes to partials + s NKV_PRESSURE_PARTIALS and
 *   sum z_s to partials + (2 + s) NKV_PRESSURE_PARTIALS.
 * nkv_pressure_pgradt / nkv_pressure_pgradt2: nkv_pressure_gradt / nkv_pressure_gradt2 for the preconditioned
 *   iteration: res (= M r) loses its mean on the load, p <- first ? res - zeta : (res - zeta) + beta p with
 *   zeta = inv_n times the sum of the B values at zsum (system s: at zsum + s*B); zsum NULL: no shift, the bits of
 *   the plain entry.  beta as there, from r.z where the plain iteration has r.r.
 * The preconditioned iteration is four launches and one dsavg batch: pgradt, div, cg_update (rr_old = the
 * partials of r.z: alpha = r.z / p.(Z E p); it emits r.r for the stop rule), precond. */
int nkv_pressure_precond(int64_t nel, int lx1, int ldim, const double* S, const double* lambda, const double* c,
                         const double* r, double* z, double* partials, void* stream);
int nkv_pressure_precond2(int64_t nel, int lx1, int ldim, const double* S, const double* lambda, const double* c,
                          const double* r0, const double* r1, double* z0, double* z1, double* partials, int active,
                          void* stream);
int nkv_pressure_pgradt(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                        const double* xm, const double* ym, const double* zm, double* p, const double* res,
                        const double* rr_new, const double* rr_old, const double* zsum, int B, double inv_n, int first,
                        double* t, int64_t t_stride, void* stream);
int nkv_pressure_pgradt2(const nkv_layout* L, int lx1, int ldim, const double* D, const double* interp, const double* gw,
                         const double* xm, const double* ym, const double* zm, double* p0, double* p1, const double* res0,
                         const double* res1, const double* rr_new, const double* rr_old, const double* zsum, int B,
                         double inv_n, int first, double* t0, double* t1, int64_t t_stride, int active, void* stream);

/* ---- shard-independent synthetic data ----------------------------------------------------
 * x[row] = 2*u - 1, u = hash(seed, field, global point) in [0,1) with 53 exact bits, for live
 * rows; padding rows = 0; time = 0.  Global point of local point i in a weighted field is
 * v_offset + i, in pressure p_offset + i (element-contiguous shards).  Bit-identical to the
 * oracle's generator for every shard split. */
int nkv_fill_hash(const nkv_layout* L, double* x, uint64_t seed, int64_t v_offset, int64_t p_offset,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEKKRYLOV_H */
