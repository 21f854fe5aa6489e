/* tmlqcd_hip.h -- C-ABI of the MI355X-native tmLQCD hot path (libtmlqcd_hip.so).
 *
 * Plain C: opaque handles, raw pointers and sizes only.  Host arrays use the
 * reference's own AoS layouts (su3.h:40-43 `su3`, su3.h:60-63 `spinor`,
 * global.h:176 `g_gauge_field[ix][mu]`, lexicographic ix of geometry_eo.c:290);
 * device-side layouts are private.
 *
 * Two layers:
 *   1. this header: explicit context + device-resident fields.  Every entry point
 *      names the reference function (file:line under /root/reference) whose
 *      semantics it reproduces.
 *   2. include/tmlqcd_dropin.h: the reference's own symbol names and signatures
 *      (Hopping_Matrix, Qtm_pm_psi, square_norm, cg_her, ...) implemented on top
 *      of layer 1 so that benchmark / invert / hmc_tm link unchanged.
 *
 * All functions returning int return 0 on success; on failure they print a
 * diagnostic to stderr and return non-zero (the drop-in layer turns that into
 * exit(), the reference's own error convention, fatal_error.c).
 */
#ifndef TMLQCD_HIP_H
#define TMLQCD_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tmhip_ctx tmhip_ctx;
typedef struct tmhip_field tmhip_field;

/* Local lattice of this rank.  Decomposition is T-only (the reference's
 * PARALLELT, mpi_init.c:240-242,330-332): global T = nproc_t * T. */
typedef struct {
  int T, LX, LY, LZ; /* local extents; all even, T >= 2 (mpi_init.c:784-799) */
  int nproc_t;       /* ranks along T (1 = single GPU, periodic wrap is local) */
  int proc_t;        /* this rank's coordinate along T */
} tmhip_geom;

enum { TMHIP_EO = 0, TMHIP_OE = 1 };           /* global.h EO/OE */
enum { TMHIP_FIELD_EO = 0, TMHIP_FIELD_FULL = 1 }; /* V/2 sites (one parity) | V sites */

/* ---- context ------------------------------------------------------------ */
/* device: HIP device ordinal.  Replaces the index-table / gauge-copy set-up of
 * geometry() (geometry_eo.c:743) + init_gauge_field (init/init_gauge_field.c:41). */
int tmhip_create(const tmhip_geom *geom, int device, tmhip_ctx **out);
void tmhip_destroy(tmhip_ctx *ctx);
int tmhip_sync(tmhip_ctx *ctx);
const char *tmhip_version(void);
int tmhip_device_count(void);

/* boundary(kappa) with X0..X3 = theta (boundary.c:40-55) */
int tmhip_set_boundary(tmhip_ctx *ctx, double kappa, const double theta[4]);
/* Same, but takes the host's ka0..ka3 verbatim (boundary.h:25) as {re0,im0,..,re3,im3}: the
 * drop-in layer re-reads the reference's globals at every call. */
int tmhip_set_ka(tmhip_ctx *ctx, const double ka[8]);
/* g_mu (global.h:198; = 2 kappa mu); read by the twisted-mass operators at call time */
int tmhip_set_mu(tmhip_ctx *ctx, double mu);
int tmhip_set_mu3(tmhip_ctx *ctx, double mu3);   /* g_mu3 (global.h:197), default 0: Qsw_plus/minus/pm_psi and Msw_plus/minus_psi twist their odd-odd
                                                  * clover term with +-(mu + mu3) (clovertm_operators.c:208,216,238,243,258,265) */

/* Upload g_gauge_field (host, su3[VOLUMEPLUSRAND][4], halo links included when
 * nproc_t > 1) and re-sort it into the device gauge copy.  Replaces
 * update_backward_gauge() (update_backward_gauge.c:185-242); call whenever
 * g_update_gauge_copy is set (Hopping_Matrix.c:135-139). */
int tmhip_set_gauge(tmhip_ctx *ctx, const void *gauge_field_lexic);

/* ---- device fields ------------------------------------------------------ */
int tmhip_field_alloc(tmhip_ctx *ctx, int kind, tmhip_field **out);
void tmhip_field_free(tmhip_ctx *ctx, tmhip_field *f);
/* host `spinor[nsites]` (AoS) <-> device.  EO fields: nsites <= V/2, e/o order of
 * geometry_eo.c:869-885.  FULL fields: nsites = V, lexicographic order. */
int tmhip_field_upload(tmhip_ctx *ctx, tmhip_field *f, const void *host_spinors, int nsites);
int tmhip_field_download(tmhip_ctx *ctx, tmhip_field *f, void *host_spinors, int nsites);
/* sites [first, first + count) of an fp64 field -> pinned_spinors[0 .. count), which must be page-locked memory (tmhip_pinned_alloc):
 * the kernel writes there directly and no staging buffer of the context is used, so this transfer alone may be issued from a second
 * host thread while another call is in progress (the fault handler of the drop-in's lazy mode).  FULL fields: first = 0, count = V. */
int tmhip_field_download_range(tmhip_ctx *ctx, tmhip_field *f, void *pinned_spinors, int first, int count);
/* page-locked host buffers (hipHostMalloc): staging for callers that keep the runtime away from their own pages */
int tmhip_pinned_alloc(unsigned long bytes, void **out);
int tmhip_pinned_free(void *p);
int tmhip_field_zero(tmhip_ctx *ctx, tmhip_field *f);
/* the planes of an fp64 one-parity field as they lie in HBM, d[12][*stride] complex doubles with the padding entries
 * [VOLUME/2, *stride): host -> device (to_device != 0) or device -> host; host == NULL only reports the stride (diagnostics, tests) */
int tmhip_field_raw(tmhip_ctx *ctx, tmhip_field *f, void *host, int to_device, int *stride);
/* FULL field <-> its two parities (linalg/convert_eo_to_lexic.c) -- views, no copy */
tmhip_field *tmhip_field_even(tmhip_field *full);
tmhip_field *tmhip_field_odd(tmhip_field *full);

/* ---- stencil (EO fields) ------------------------------------------------ */
/* Hopping_Matrix(ieo, l, k)            operator/Hopping_Matrix.c:131-156 */
int tmhip_hopping_matrix(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k);
/* Hopping_Matrix_nocom                  operator/Hopping_Matrix_nocom.c:48-56 (halo exchange skipped) */
int tmhip_hopping_matrix_nocom(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k);
/* tm_times_Hopping_Matrix(ieo,l,k,c)    operator/tm_times_Hopping_Matrix.c:72 ; epilogue hopping.h:674-678 */
int tmhip_tm_times_hopping_matrix(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k, double cre, double cim);
/* tm_sub_Hopping_Matrix(ieo,l,p,k,c)    operator/tm_sub_Hopping_Matrix.c:73 ; epilogue hopping.h:680-688 */
int tmhip_tm_sub_hopping_matrix(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *p, tmhip_field *k,
                                double cre, double cim);
/* D_psi(P,Q) on FULL fields             operator/D_psi.c:1133-1140, D_psi_body.c:266-375 */
int tmhip_D_psi(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q);

/* ---- site-diagonal twisted-mass ops (operator/tm_operators.h:26-77) ------ */
int tmhip_mul_one_pm_imu_inv(tmhip_ctx *ctx, tmhip_field *l, double sign, int N);
int tmhip_assign_mul_one_pm_imu_inv(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, double sign, int N);
int tmhip_assign_mul_one_pm_imu(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, double sign, int N);
int tmhip_mul_one_pm_imu(tmhip_ctx *ctx, tmhip_field *l, double sign);
int tmhip_mul_one_pm_imu_sub_mul(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j, double sign, int N);
int tmhip_mul_one_pm_imu_sub_mul_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j, double sign);
int tmhip_mul_one_sub_mul_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j); /* tm_operators.c:781-810 */
int tmhip_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, int N); /* gamma.c:77-98 */

/* ---- e/o compositions (operator/tm_operators.c) -------------------------- */
int tmhip_H_eo_tm_inv_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, int ieo, double sign); /* :508-526 */
int tmhip_Qtm_plus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);   /* :172-177 */
int tmhip_Qtm_minus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);  /* :216-221 */
int tmhip_Mtm_plus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);   /* :245-250 */
int tmhip_Mtm_minus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);  /* :289-294 */
int tmhip_Qtm_pm_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);     /* :338-345 */
int tmhip_M_full(tmhip_ctx *ctx, tmhip_field *Even_new, tmhip_field *Odd_new,
                 tmhip_field *Even, tmhip_field *Odd);                    /* :117-128 */
/* symmetric e/o preconditioning  1 - A^-1 H_oe A^-1 H_eo  (non-hermitian solvers of invert_eo.c:177-280) */
int tmhip_Qtm_plus_sym_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);      /* :186-192 */
int tmhip_Qtm_minus_sym_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);     /* :223-229 */
int tmhip_Mtm_plus_sym_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);      /* :259-265 */
int tmhip_Mtm_minus_sym_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);     /* :296-302 */
int tmhip_Mtm_plus_sym_dagg_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k); /* :312-322, l != k */
int tmhip_Qtm_pm_sym_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);        /* :347-364 (returns what the reference returns) */

/* ---- spinor linalg (linalg/ of the reference) ---------------------------- */
/* `parallel` != 0 adds the cross-rank sum (MPI_Allreduce in the reference). */
int tmhip_square_norm(tmhip_ctx *ctx, tmhip_field *P, int N, int parallel, double *out);                       /* square_norm.c:253 */
int tmhip_scalar_prod_r(tmhip_ctx *ctx, tmhip_field *S, tmhip_field *R, int N, int parallel, double *out);     /* scalar_prod_r.c:135 */
int tmhip_assign_add_mul_r(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, double c, int N);                   /* assign_add_mul_r.c:346 */
int tmhip_assign_mul_add_r(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N);                   /* assign_mul_add_r.c:340 */
int tmhip_assign_add_mul(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, double c_re, double c_im, int N);     /* linalg/assign_add_mul.c: P += c Q, complex c; P may be Q */
int tmhip_assign_mul_add_r_and_square(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N,
                                      int parallel, double *out);                                             /* assign_mul_add_r_and_square.c:145 */
int tmhip_diff(tmhip_ctx *ctx, tmhip_field *Q, tmhip_field *R, tmhip_field *S, int N);                         /* diff.c:270 */
int tmhip_assign(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, int N);                                       /* assign.c:42 */
int tmhip_add(tmhip_ctx *ctx, tmhip_field *Q, tmhip_field *R, tmhip_field *S, int N);                          /* linalg/add.c:45   Q = R + S */
int tmhip_mul_r(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N);                              /* linalg/mul_r.c:40 R = c S */
/* Complex singles: out = {Re, Im} of sum conj(S) R (linalg/scalar_prod_body.c:52), both parts from one launch; R -= c S; R = c S (R may be S).
 * They are the one-field instances of the batched kernels below, so a batched value carries the bits of its single. */
int tmhip_scalar_prod(tmhip_ctx *ctx, tmhip_field *S, tmhip_field *R, int N, int parallel, double out[2]);     /* linalg/scalar_prod.c */
int tmhip_assign_diff_mul(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, double c_re, double c_im, int N);    /* linalg/assign_diff_mul.c */
int tmhip_mul(tmhip_ctx *ctx, tmhip_field *R, double c_re, double c_im, tmhip_field *S, int N);                /* linalg/mul.c */
/* Batched forms, 1 <= n <= TMHIP_CSG_MAX fields, unsplit fp64 EO fields; coefficients and results are (re, im) pairs.
 *   multi_scalar_prod     out[i] = <S_i, R> in one pass over R (groups of six S_i per launch), ONE final-reduction launch, one copy to
 *                         the host and one synchronisation; rank-local: a context that sums over ranks refuses it
 *   multi_assign_diff_mul R_i -= c_i S for all i, S read once per group
 *   lincomb               P = sum_i c_i V_i, every element added up from i = n-1 down to 0 (chrono_guess.c:144-153) */
#define TMHIP_CSG_MAX 20
int tmhip_multi_scalar_prod(tmhip_ctx *ctx, int n, tmhip_field *const *S, tmhip_field *R, int N, double *out /* 2n */);
int tmhip_multi_assign_diff_mul(tmhip_ctx *ctx, int n, tmhip_field *const *R, tmhip_field *S, const double *c /* 2n */, int N);
int tmhip_lincomb(tmhip_ctx *ctx, tmhip_field *P, int n, tmhip_field *const *V, const double *c /* 2n */, int N);

/* ---- solver --------------------------------------------------------------- */
/* The operators a solver takes as `op`, by the reference's function.  Which field kind an id acts on, whether it needs a valid clover
 * term and which solvers take it is ONE list, tmlqcd_amd/csrc/op_table.h; a solver refuses, with a message and before it writes
 * anything, an id outside that list, an id that is not in its column, fields of another kind than the row's, and a clover row on a
 * context without a valid clover term. */
enum { TMHIP_OP_QTM_PM = 0, TMHIP_OP_QTM_PLUS = 1, TMHIP_OP_QTM_MINUS = 2, TMHIP_OP_MTM_PLUS = 3, TMHIP_OP_MTM_MINUS = 4,
       TMHIP_OP_QSW_PM = 5 /* Qsw_pm_psi */,
       TMHIP_OP_Q_PM_FULL = 6 /* Q_pm_psi on FULL fields (tm_operators.c:380-388) */,
       TMHIP_OP_MTM_PLUS_SYM = 7, TMHIP_OP_MTM_MINUS_SYM = 8 /* Mtm_plus/minus_sym_psi */,
       TMHIP_OP_QSW_PLUS = 9, TMHIP_OP_QSW_MINUS = 10, TMHIP_OP_MSW_PLUS = 11 /* Qsw_plus/minus_psi, Msw_plus_psi */,
       TMHIP_OP_D_PSI = 12 /* D_psi on FULL fields, N = VOLUME */ };
/* cg_her(P,Q,max_iter,eps_sq,rel_prec,N,f)   solver/cg_her.c:62-141.
 * Device-resident: P, Q and the three work fields never leave HBM.  Returns the
 * iteration count in *iters (-1 if not converged); res_hist (may be NULL) gets
 * err after each iteration, up to hist_len entries. */
int tmhip_cg_her(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, int max_iter, double eps_sq, int rel_prec,
                 int N, int op, int *iters, double *res_hist, int hist_len);

/* ---- BiCGstab (solver/bicgstab_complex.c:49-116) ------------------------------
 * The two three-field complex singles of its loop, on fp64 fields of one kind: EO fields with 0 <= N <= VOLUME/2 or FULL fields with
 * N = VOLUME.  Element-wise, so R may be S or U.  The four products of a complex product are rounded one by one: every element carries
 * the bits of the reference's statement.
 *   assign_add_mul_add_mul          R += c1 S + c2 U          (linalg/assign_add_mul_add_mul.c:42-60)
 *   assign_mul_bra_add_mul_ket_add  R = c2 (R + c1 S) + U     (linalg/assign_mul_bra_add_mul_ket_add.c:44-63) */
int tmhip_assign_add_mul_add_mul(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, double c1_re, double c1_im, double c2_re,
                                 double c2_im, int N);
int tmhip_assign_mul_bra_add_mul_ket_add(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, double c1_re, double c1_im, double c2_re,
                                         double c2_im, int N);
/* bicgstab_complex(P,Q,max_iter,eps_sq,rel_prec,N,f): P is the starting guess and receives the solution, *iters the reference's return
 * value (i, or -1 after max_iter iterations or on the breakdown of :102).  op: the rows of the operator table that name this solver,
 * on EO fields with N = VOLUME/2 or on FULL fields with N = VOLUME as the row says.  res_hist (may
 * be NULL) gets |r|^2 at the top of every iteration the reference runs, entry 0 being the starting residual: up to iters + 1 entries.
 * Six work fields of the context per field kind are allocated on first use and freed with the context.
 * Option "bicg_fused" (tmhip_set_option) 1 (default): the five fused kernels K1-K5 of bicgstab.hip with the scalars in a device state block
 * and no host synchronisation but the poll; 0: the reference's statement sequence on the singles, one host round trip per scalar.
 * Refused with a message, P and *iters untouched: a T-split context or its loopback rehearsal, fp32 fields, a field kind or an N that does
 * not match the operator, a clover operator without a valid clover term. */
int tmhip_bicgstab_complex(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, int max_iter, double eps_sq, int rel_prec, int N, int op,
                           int *iters, double *res_hist, int hist_len);
/* The fused kernels alone, with the scalars handed over by the host (the solver's kernels read them from its device state): given the same
 * scalars each leaves the bits of the singles it replaces, each sum the bits of tmhip_scalar_prod / tmhip_square_norm of the same fields
 * (FULL fields: of the two halves, added even first).  Fields of one kind, N as for the solver, no two fields of a call may be one.
 *   bicg_update    K4: P += alpha p + omega s ; r = s - omega t ; out = {Re <hatr, r>, Im <hatr, r>, <r, r>}
 *   bicg_pair_dot  K3: out = {Re <t, s>, Im <t, s>, <t, t>} in one pass over t
 *   bicg_sub       K2: s = r - alpha v
 *   bicg_dir       K5: p = beta (p - omega v) + r */
int tmhip_bicg_update(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *r, tmhip_field *p, tmhip_field *s, tmhip_field *t, tmhip_field *hatr,
                      const double alpha[2], const double omega[2], int N, double out[3]);
int tmhip_bicg_pair_dot(tmhip_ctx *ctx, tmhip_field *t, tmhip_field *s, int N, double out[3]);
int tmhip_bicg_sub(tmhip_ctx *ctx, tmhip_field *s, tmhip_field *r, tmhip_field *v, const double alpha[2], int N);
int tmhip_bicg_dir(tmhip_ctx *ctx, tmhip_field *p, tmhip_field *v, tmhip_field *r, const double omega[2], const double beta[2], int N);

/* ---- chronological solver guess (solver/chrono_guess.c) ---------------------
 * tmhip_chrono_guess: the starting vector of A x = phi from the last n normalised solutions v[0..n-1] (oldest first, i.e. already in
 * index_array order), A = operator `op` (TMHIP_OP_*), N sites of EO fields:
 *   1. every older vector is made orthogonal to the newest one, v_i -= <v_{n-1}, v_i> v_{n-1} for i < n-1 (the caller's v_i change);
 *   2. G[i][j] = <v_i, A v_j> is computed for i <= j and mirrored, G[j][i] = conj(G[i][j]); b[j] = <v_j, phi>;
 *   3. G y = b is solved on the host by a row-wise LU factorisation with partial pivoting;
 *   4. trial = sum_i y_i v_i.
 * n = 0 or N = 0 gives trial = 0; n > TMHIP_CSG_MAX is an error.  G_out (2 n n doubles, row-major) and b_out (2 n doubles, the
 * projections of step 2) may be NULL.  Option "csg_batch" 1 (default): steps 1, 2 and 4 run on the batched kernels (n + 2 host
 * synchronisations instead of (n-1) + n(n+1)/2 + n); 0, a rank that sums over ranks, or N != VOLUME/2: the same steps as a sequence of
 * the complex singles with the cross-rank sum.
 * tmhip_chrono_add_solution: slot = trial / |trial| (square_norm over all ranks, then mul_r). */
int tmhip_chrono_guess(tmhip_ctx *ctx, tmhip_field *trial, tmhip_field *phi, tmhip_field *const *v, int n, int op, int N,
                       double *G_out, double *b_out);
int tmhip_chrono_add_solution(tmhip_ctx *ctx, tmhip_field *slot, tmhip_field *trial, int N);
/* step 3 alone, on the host: G (2 n n doubles, row-major, overwritten with its factors) y = b, y returned in b (2 n doubles); 1 <= n <= TMHIP_CSG_MAX */
int tmhip_csg_solve(int n, double *G, double *b);

/* ---- eigenvalue measurement (solver/eigenvalues.c, solver/eigenvalues_bi.c, phmc.c:205-253) -----------------
 * The nev lowest (which = 0) or highest (which = 1) eigenpairs of a Hermitian positive operator by thick-restart Lanczos (Wu and
 * Simon) with full reorthogonalisation (classical Gram-Schmidt, twice), where the reference runs Jacobi-Davidson on LAPACK with host
 * vectors.  fp64, unsplit lattices.  The basis of a cycle has m = "eig_basis" vectors (tmhip_set_option; nev + 2 <= m <=
 * TMHIP_EIG_MAX_BASIS), a restart keeps nev + (m - nev) / 2 Ritz vectors (at most m - 2) and the residual vector.  The small
 * symmetric eigenproblem is solved on the host (tmhip_eig_small: cyclic Jacobi, csrc/eig_small.h).
 *   tmhip_eigenvalues     op: the rows of the operator table marked TMHIP_S_EIG -- Qtm_pm_psi, Qsw_pm_psi (valid clover term) on EO
 *                         fields with N = VOLUME/2, Q_pm_psi on FULL fields with N = VOLUME
 *   tmhip_eigenvalues_nd  op: TMHIP_ND_OP_* (the doublet rows); a vector is the pair (up, dn)
 * evals[0 .. nev): ascending for which = 0, descending for which = 1; each is the Rayleigh quotient <v, A v> of its Ritz vector with
 * the operator itself, resid[i] = |A v_i - evals[i] v_i| with |v_i| = 1, computed, not estimated.  *converged = how many of the nev
 * pairs have resid <= prec (an absolute bound, as tol of jdher); the run ends when all have.  max_apps (>= nev + 1) caps the
 * operator applications, those of the residuals included; reaching it is no error: the call returns 0 with *converged < nev and the
 * best estimates with their residuals (a pair the cap left no vector for comes back with resid = infinity).  *apps = applications done.
 * evec (evec_up, evec_dn), NULL or nev fields of the operator's kind: on exit evec[i] is the unit eigenvector of evals[i].  ON ENTRY
 * evec[0] is the start vector if its norm is not zero; otherwise (and with evec = NULL) a fixed pseudo-random vector starts the run.
 * One start vector finds ONE eigenvector per distinct eigenvalue: exact multiplicities (the doublet at epsbar = 0) are not promised,
 * a degenerate eigenvalue is reported once and the next distinct one follows.
 * Option "eig_cheb" = d > 0 (default 4): the lowest end runs on B = T_d((hi + lo - 2 A) / (hi - lo)), whose largest eigenvalues are the wanted
 * ones; eigenvalues and residuals are still those of A.  tmhip_eig_set_interval gives (lo, hi), 0 < lo < hi with every wanted
 * eigenvalue below lo and the spectrum below hi; (0, 0), the default, takes them from one unfiltered cycle: hi = 1.1 (largest Ritz
 * value + its residual bound), lo = the largest Ritz value the restart rule would keep.  The highest end always runs unfiltered.
 * Option "eig_fused" 1 (default): tmhip_eig_dots / _eig_project / _basis_rotate, the coefficients never leave the device: a step is nine
 * launches beside the operator (dots, project, dots, project, each with its one-block final pass, and the scaling to unit norm as a
 * pass of its own) with one host synchronisation, and none inside the filter; 0: the same algorithm on tmhip_multi_scalar_prod (calls
 * of up to TMHIP_CSG_MAX = 20 fields, six per launch inside), tmhip_multi_assign_diff_mul per vector, tmhip_square_norm, tmhip_mul_r and,
 * for the rotation, tmhip_lincomb into work vectors, with their host round trips (the baseline of tools/eig_speed.py, the cross-check
 * of the tests; its rotation holds up to m - 2 more vectors while it runs).  Neither form changes bits from call to call.
 * Not built, so not measured against what is: the scaling folded into the second projection, and a rotation that walks its outputs in
 * column groups (the rotation keeps all k accumulators of a thread in registers: 8 / 6 / 3 / 1 waves per SIMD for k <= 8 / 16 / 32 / 64).
 * Work memory: m + 3 vectors (m + 1 basis, 2 work), allocated on first use, kept for the next call and freed with the context -- a
 * vector being one EO field, one FULL field or two EO fields -- plus 2 * 65 block sums per block of a launch.
 * Refused with a message, nothing written: an operator outside the rows above (tmhip_op_check / tmhip_nd_op_check), a clover row
 * without its clover term, an N or fields that do not match the operator, nev + 2 > "eig_basis", a T-split context or its loopback
 * rehearsal.
 * Not built: T-split ranks, fp32 and mixed precision, block Lanczos, interior eigenvalues. */
#define TMHIP_EIG_MAX_BASIS 64
int tmhip_eigenvalues(tmhip_ctx *ctx, int op, int N, int nev, int which /* 0 lowest, 1 highest */, double prec, int max_apps,
                      tmhip_field *const *evec /* nev fields or NULL */, double *evals, double *resid, int *converged, int *apps);
int tmhip_eigenvalues_nd(tmhip_ctx *ctx, int op, int nev, int which, double prec, int max_apps, tmhip_field *const *evec_up,
                         tmhip_field *const *evec_dn /* both nev fields, or both NULL */, double *evals, double *resid, int *converged, int *apps);
int tmhip_eig_set_interval(tmhip_ctx *ctx, double lo, double hi);   /* 0, 0 = automatic */
/* The pieces, public so that they can be tested.  A vector is v_up[i] alone (v_dn = NULL, w_dn = NULL: EO fields with 1 <= N <= VOLUME/2
 * sites, or FULL fields with N = VOLUME) or the pair (v_up[i], v_dn[i]) of EO fields; all of one kind.
 *   eig_dots      out[2i], out[2i+1] = Re, Im <v_i, w>, i < nv <= 65, in ONE launch that reads w once and every v_i once; an EO value
 *                 carries the bits of tmhip_scalar_prod of the same pair (a pair of flavours: of the up value + the down value)
 *   eig_project   w -= sum_i h_i v_i (h: nv complex coefficients), added up in ascending i; *sqnorm = |w|^2 of the result from the
 *                 same pass.  w may not be one of the v_i.
 *   basis_rotate  V[:, 0:k] = V[:, 0:n] Y in place, Y real n x k row-major, 1 <= k <= n <= TMHIP_EIG_MAX_BASIS; vectors k .. n-1
 *                 are left as they are
 *   eig_small     host only: A (n x n symmetric, row-major, n <= TMHIP_EIG_MAX_BASIS) -> its eigenvectors by column, w ascending */
int tmhip_eig_dots(tmhip_ctx *ctx, int nv, tmhip_field *const *v_up, tmhip_field *const *v_dn, tmhip_field *w_up, tmhip_field *w_dn, int N,
                   double *out /* 2 nv */);
int tmhip_eig_project(tmhip_ctx *ctx, int nv, tmhip_field *const *v_up, tmhip_field *const *v_dn, tmhip_field *w_up, tmhip_field *w_dn,
                      const double *h /* 2 nv */, int N, double *sqnorm);
int tmhip_basis_rotate(tmhip_ctx *ctx, int n, int k, tmhip_field *const *v_up, tmhip_field *const *v_dn, const double *Y /* n * k */, int N);
int tmhip_eig_small(int n, double *A /* n*n, in: symmetric, out: eigenvectors by column */, double *w);

/* ---- LapH eigensystem: the gauge-covariant 3D Laplacian on all time-slices (jacobi.c, LapH_ev.c, solver/eigenvalues_Jacobi.c) -----
 * A colour-vector field is T x LX LY LZ sites of three complex doubles, no spin: one 3D lattice per time-slice.  Host image: the
 * reference's su3_vector [T][SPACEVOLUME], t slowest, then x, y, z (the ix of geometry_eo.c:851-860; t SPACEVOLUME + ix is the
 * lexicographic site of g_gauge_field).  Device: three colour planes of VOLUME sites at a stride, a time-slice is a contiguous range
 * of every plane.  Unsplit contexts only.
 *   tmhip_laph_apply        out[t] = Jacobi(in[t], t) of jacobi.c:43-72 for t0 <= t < t0 + nt in ONE launch:
 *                           l(x) = 6 k(x) - sum_{mu=1..3} [ U_mu(x) k(x+mu) + U_mu(x-mu)^dagger k(x-mu) ], the subtractions in the
 *                           reference's order, on the raw resident links (no boundary phases, no kappa), neighbours wrap inside the
 *                           slice (an extent of 2: x+mu and x-mu are one site and both terms count).  out != in.  Slices outside the
 *                           range are not touched.  The links are the lexicographic copy tmhip_set_gauge left and tmhip_update_gauge /
 *                           tmhip_gauge_restore keep current.
 *   tmhip_laph_apply_dot    the same and dots[2 t'], dots[2 t' + 1] = Re, Im <in, out> of slice t0 + t' from the same pass
 *   tmhip_laph_apply_filter out = c1 (A in) + c2 in + c3 prev with coef[3 t' ..] = (c1, c2, c3) of slice t0 + t': the Chebyshev
 *                           three-term step, no vector pass of its own.  prev may be NULL (c3 is then not read); out differs from in
 *                           and prev.
 * Options: "laph_basis" 0 (default: m = nev + 32, at most TMHIP_LAPH_MAX_BASIS) or m itself; "laph_cheb" 16 (default) the degree of the
 * filter, 0 none -- the fastest of tools/laph_speed.py, profiles/r22_laph_speed.log.  "laph_fused" 1 (default): one stencil launch per call.  0: the plain operator and a separate pass (the dots / the
 * combination), the cross-check and the baseline of tools/laph_speed.py.
 * The batched Lanczos pieces, public so that they can be tested: the time-slice is a grid dimension, every scalar is an array over the
 * slices of the range that stays on the device inside the driver.  active: NULL, or nt flags; a slice whose flag is 0 is frozen --
 * its blocks return at once, nothing of it is read or written and its entries of the outputs are left as they were.  Every sum is
 * added in a fixed order (one partial per block, a fixed final pass): the same bits from call to call.
 *   tmhip_laph_dots      out[(t' nv + i) 2 ..] = Re, Im <v_i, w> of slice t0 + t', i < nv <= TMHIP_LAPH_MAX_BASIS + 1; a launch takes up
 *                        to 65 vectors (w once, each v_i once), more are taken in chunks
 *   tmhip_laph_project   w[t] -= sum_i h[t'][i] v_i[t], ascending i (h as tmhip_laph_dots leaves it); sqnorm[t'] = |w[t]|^2 of the
 *                        result from the same pass.  nv = 0: the norms alone.  w may not be one of the v_i.
 *   tmhip_laph_normalise out[t] = in[t] / |in[t]| (zero for a slice of norm zero); sqnorm[t'] = |in[t]|^2.  out may be in.
 *   tmhip_laph_rotate    V[t][:, 0:k] = V[t][:, 0:n] Y_t in place, Y real [nt][n][k], 1 <= k <= n <= TMHIP_LAPH_MAX_BASIS: an
 *                        element's n values wait in LDS while the k columns are formed in groups of 16; vectors k .. n-1 stay
 * The driver: tmhip_laph_eigensystem returns the nev lowest eigenpairs of every slice of the range.  Per slice the algorithm is exactly
 * that of tmhip_eigenvalues with which = 0 (tests/eig_restate.py is its statement): thick restart keeping nev + (m - nev) / 2 of the
 * m = "laph_basis" vectors, classical Gram-Schmidt twice, convergence on the true residual against the absolute prec, the Chebyshev
 * filter of degree "laph_cheb" on the lowest end with the interval per slice from one unfiltered cycle by the same rule or from
 * tmhip_laph_set_interval, max_apps the cap of applications per slice (reaching it is no error).  All slices advance in lock-step: one
 * launch of every kernel and ONE host synchronisation per Lanczos step for all of them, none inside the filter; a slice that has
 * converged, hit its cap or met an invariant subspace is frozen while the others finish.  The nt small eigenproblems of a restart are
 * solved on up to 16 host threads (cyclic Jacobi, csrc/eig_small.h).
 *   evec       NULL or nev colour-vector fields: evec[i] holds eigenvector i of every slice of the range, unit norm per slice.  ON ENTRY
 *              evec[0] is the start vector of every slice where its norm is non-zero; a fixed pseudo-random fill starts the others.
 *   evals      [nt][nev], ascending: Rayleigh quotients with the operator itself;  resid [nt][nev]: the computed |A v - theta v|
 *   converged  [nt]: pairs with resid <= prec;  apps [nt]: operator applications of the slice
 * Work memory: m + 3 colour-vector fields, allocated on first use, kept, freed with the context.
 * tmhip_laph_write writes what the non-MPI branch of eigenvalues_Jacobi.c:176-209 writes into `dir`: eigenvalues.%.3d.%.4d (tslice,
 * nstore) with one "%e\n" line per eigenvalue, eigenvector.%.3d.%.3d.%.4d (ev, tslice, nstore) with the raw host-order image of the
 * slice, SPACEVOLUME x 3 complex doubles, no header.
 * Refused with a message, nothing written: T-split contexts and their loopback rehearsal, no resident links, a slice range outside
 * [0, T) or of more than 256 slices, nev + 2 > "laph_basis", out == in, fields of another context.
 * Not built: T-split ranks, fp32 or mixed precision, Lemon / MPI output, more than 126 eigenpairs per slice, exact multiplicities (one
 * start vector finds one eigenvector per distinct eigenvalue), link smearing (upload smeared links), cg_her_su3vect / jdher_su3vect. */
#define TMHIP_LAPH_MAX_BASIS 128
typedef struct tmhip_cvfield tmhip_cvfield;
int tmhip_cvfield_alloc(tmhip_ctx *ctx, tmhip_cvfield **out);   /* zeroed */
void tmhip_cvfield_free(tmhip_ctx *ctx, tmhip_cvfield *f);
int tmhip_cvfield_upload(tmhip_ctx *ctx, tmhip_cvfield *f, const void *host /* [T][SPACEVOLUME][3] complex double */);
int tmhip_cvfield_download(tmhip_ctx *ctx, tmhip_cvfield *f, void *host);
/* the slices [t0, t0 + nt) alone: host holds [nt][SPACEVOLUME][3] complex double */
int tmhip_cvfield_upload_slices(tmhip_ctx *ctx, tmhip_cvfield *f, const void *host, int t0, int nt);
int tmhip_cvfield_download_slices(tmhip_ctx *ctx, tmhip_cvfield *f, void *host, int t0, int nt);
int tmhip_cvfield_zero(tmhip_ctx *ctx, tmhip_cvfield *f);
int tmhip_laph_apply(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt);
int tmhip_laph_apply_dot(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt, double *dots /* [nt][2] */);
int tmhip_laph_apply_filter(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, tmhip_cvfield *prev /* or NULL */, int t0, int nt,
                            const double *coef /* [nt][3] */);
int tmhip_laph_dots(tmhip_ctx *ctx, int nv, tmhip_cvfield *const *v, tmhip_cvfield *w, int t0, int nt, const int *active /* nt or NULL */,
                    double *out /* [nt][nv][2] */);
int tmhip_laph_project(tmhip_ctx *ctx, int nv, tmhip_cvfield *const *v, tmhip_cvfield *w, const double *h /* [nt][nv][2] */, int t0, int nt,
                       const int *active, double *sqnorm /* [nt] */);
int tmhip_laph_normalise(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt, const int *active, double *sqnorm /* [nt] */);
int tmhip_laph_rotate(tmhip_ctx *ctx, int n, int k, tmhip_cvfield *const *v, const double *Y /* [nt][n][k] */, int t0, int nt, const int *active);
int tmhip_laph_set_interval(tmhip_ctx *ctx, double lo, double hi);   /* of every slice; 0, 0 = automatic, per slice */
int tmhip_laph_eigensystem(tmhip_ctx *ctx, int t0, int nt, int nev, double prec, int max_apps, tmhip_cvfield *const *evec /* nev fields or NULL */,
                           double *evals, double *resid, int *converged, int *apps);
/* host seconds of the last tmhip_laph_eigensystem: out[0] in the small eigenproblems, out[1] in the whole call (tools/laph_speed.py) */
int tmhip_laph_timing(tmhip_ctx *ctx, double out[2]);
int tmhip_laph_write(tmhip_ctx *ctx, const char *dir, int nstore, int t0, int nt, int nev, tmhip_cvfield *const *evec, const double *evals /* [nt][nev] */);

/* ---- non-degenerate twisted-mass doublet (operator/tm_operators_nd.c) ------------------------
 * A doublet is a pair of EO fields (strange = up, charm = dn).  Unsplit lattices only: a context with nproc_t > 1 refuses every
 * entry point below with a message.  Wilson twisted mass, fp64, no clover term (the clover doublet and the fp32 twins follow below). */
/* g_mubar, g_epsbar (global.h:202) and phmc_invmaxev (phmc.h:31; default 1), read by the operators and solvers at call time */
int tmhip_set_nd(tmhip_ctx *ctx, double mubar, double epsbar, double invmaxev);
/* M_ee_inv_ndpsi(l_s,l_c,k_s,k_c,mu,eps)          tm_operators_nd.c:639-696; l may be k */
int tmhip_M_ee_inv_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double mu, double eps);
/* M_oo_sub_g5_ndpsi(l_s,l_c,k_s,k_c,j_s,j_c,mu,eps)  :698-757; l may be k or j */
int tmhip_M_oo_sub_g5_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *j_s,
                            tmhip_field *j_c, double mu, double eps);
int tmhip_Qtm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);          /* :68-89 */
int tmhip_Qtm_dagger_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);   /* :130-152 */
int tmhip_Qtm_pm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);       /* :195-238; l may be k */
int tmhip_H_eo_tm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, int ieo);   /* :508-519 */
/* Q_tau1_sub_const_ndpsi(l_s,l_c,k_s,k_c,z,Cpol,invev)   :311-380: l = Cpol invev Qhat tau^1 k - Cpol z k with g_mubar, g_epsbar of
 * tmhip_set_nd (invev is the argument, as in the reference); two stencil launches, the constant in the epilogue of the second; l != k */
int tmhip_Q_tau1_sub_const_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double z_re, double z_im,
                                 double Cpol, double invev);
/* cg_her_nd(P_up,P_dn,Q_up,Q_dn,max_iter,eps_sq,rel_prec,N,Qtm_pm_ndpsi)   solver/cg_her_nd.c:57-160; *iters = its return value */
int tmhip_cg_her_nd(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                    int rel_prec, int N, int *iters);
/* cg_mms_tm_nd(Pup,Pdn,Qup,Qdn,solver_params) with M_ndpsi = Qtm_pm_ndpsi   solver/cg_mms_tm_nd.c:64-215: Pup[s], Pdn[s] solve
 * (Qtm_pm_ndpsi + shifts[s]^2) P = Q for s = 0 .. nshifts-1 (1 <= nshifts <= 32); the last shift is dropped every 20 iterations once
 * its correction is below eps_sq (:158-167); *iters = the reference's return value (:208-209) */
int tmhip_cg_mms_tm_nd(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts,
                       int nshifts, int max_iter, double eps_sq, int rel_prec, int *iters);
/* shifts still active at the end of the last tmhip_cg_mms_tm_nd (the reference's local `shifts`, cg_mms_tm_nd.c:68,163) */
int tmhip_nd_active_shifts(tmhip_ctx *ctx);

/* ---- the clover doublet (Qsw_*_ndpsi of operator/tm_operators_nd.c, the _nd functions of operator/clovertm_operators.c) ----------
 * Unsplit lattices, fp64: a T-split context or its loopback rehearsal is refused with a message before any launch.  The caller has run
 * tmhip_sw_term and tmhip_sw_invert_nd(mubar^2 - epsbar^2) on the current links; whatever invalidates the clover term (tmhip_sw_term,
 * tmhip_set_clover, tmhip_update_gauge, an ILDG read) drops sw_inv_nd with it, and every consumer then refuses with a message.
 * mubar, epsbar and phmc_invmaxev come from tmhip_set_nd.  "nd_fused" 1 / 0 selects the doublet stencil with the clover mixing as its
 * epilogue / two single-flavour stencils and one site-local pass, as for the twisted-mass doublet. */
/* sw_invert_nd(mshift)   operator/clover_invert.c:440-495: ((1+T)^2 + mshift)^-1 on the even sites.  Deviation: the reference overwrites
 * sw_inv; here the result lives in an array of its own (all four 3x3 blocks per chirality, 1152 bytes per even site), so cloverdet and
 * ndcloverrat alternate without inverting again.  tmhip_get_clover_nd returns it as su3 sw_inv[VOLUME/2][4][2].
 * tmhip_sw_invert_nd and tmhip_sw_deriv_nd are site-local and run on T-split contexts too; every operator, solver and monomial refuses. */
int tmhip_sw_invert_nd(tmhip_ctx *ctx, double mshift);
int tmhip_get_clover_nd(tmhip_ctx *ctx, void *sw_inv_host);
/* near-singular pivots met by the last tmhip_sw_invert / tmhip_sw_invert_nd (six_invert's error count; the reference prints it) */
int tmhip_sw_invert_failures(tmhip_ctx *ctx, int *fails);
/* assign_mul_one_sw_pm_imu_eps(ieo,k_s,k_c,l_s,l_c,mu,eps)   clovertm_operators.c:960-1074; k may be l */
int tmhip_assign_mul_one_sw_pm_imu_eps(tmhip_ctx *ctx, int ieo, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *l_s, tmhip_field *l_c, double mu,
                                       double eps);
/* clover_inv_nd(ieo,l_c,l_s)   :352-425, in place, ieo = EE only (sw_invert_nd inverts the even sites) */
int tmhip_clover_inv_nd(tmhip_ctx *ctx, int ieo, tmhip_field *l_c, tmhip_field *l_s);
/* clover_gamma5_nd(ieo,l_c,l_s,k_c,k_s,j_c,j_s,mubar,epsbar)   :733-850; l may be k or j */
int tmhip_clover_gamma5_nd(tmhip_ctx *ctx, int ieo, tmhip_field *l_c, tmhip_field *l_s, tmhip_field *k_c, tmhip_field *k_s, tmhip_field *j_c,
                           tmhip_field *j_s, double mubar, double epsbar);
int tmhip_Qsw_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);          /* tm_operators_nd.c:91-111 */
int tmhip_Qsw_dagger_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);   /* :154-174 */
int tmhip_Qsw_pm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);       /* :240-285; l may be k */
/* Qsw_tau1_sub_const_ndpsi(l_s,l_c,k_s,k_c,z,Cpol,invev)   :378-444, statement by statement (the swapped output order of :393-395 included); l != k */
int tmhip_Qsw_tau1_sub_const_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double z_re, double z_im,
                                   double Cpol, double invev);
int tmhip_H_eo_sw_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);      /* :521-535; l may be k */
int tmhip_Msw_ee_inv_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);   /* :539-549; l may be k */
/* The doublet solvers on either operator: op = TMHIP_ND_OP_QTM_PM (the un-suffixed calls above, bit for bit) or TMHIP_ND_OP_QSW_PM
 * (f / M_ndpsi = Qsw_pm_ndpsi).  One engine, one state, one polling loop. */
enum { TMHIP_ND_OP_QTM_PM = 0, TMHIP_ND_OP_QSW_PM = 1 };
int tmhip_cg_her_nd_op(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                       int rel_prec, int N, int op, int *iters);
int tmhip_cg_mms_tm_nd_op(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts,
                          int nshifts, int max_iter, double eps_sq, int rel_prec, int op, int *iters);
/* ---- the fp32 doublet and the mixed-precision doublet solve (operator/tm_operators_nd_32.c, solver/rg_mixed_cg_her_nd.c) ----------
 * Wilson twisted mass on unsplit lattices: a T-split context or its loopback rehearsal is refused with a message before any launch.
 * The operators act on fp32 EO fields (tmhip_field_alloc32) and read the fp32 twin of the links, built on first use.  mu, eps, nrm and
 * phmc_invmaxev^2 are rounded to float as the reference's casts do.  The doublet stencil reads every link in full, 18 reals, whatever
 * "gauge_recon" says.  "nd_fused" 1 (default) / 0: one doublet stencil per hop with the mixing as its epilogue / two
 * tmhip_hopping_matrix_32 launches per hop and one mixing kernel, the same operator. */
/* M_ee_inv_ndpsi_32(l_s,l_c,k_s,k_c,mu,eps)   tm_operators_nd_32.c:137-149; l may be k */
int tmhip_M_ee_inv_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, float mu, float eps);
/* M_oo_sub_g5_ndpsi_32(l_s,l_c,k_s,k_c,j_s,j_c,mu,eps)   :200-213; l may be k or j */
int tmhip_M_oo_sub_g5_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *j_s,
                               tmhip_field *j_c, float mu, float eps);
/* Qtm_pm_ndpsi_32(l_s,l_c,k_s,k_c)   :215-263 with mubar, epsbar, invmaxev of tmhip_set_nd: four launches; l may be k */
int tmhip_Qtm_pm_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c);
/* rg_mixed_cg_her_nd(P_up,P_dn,Q_up,Q_dn,solver_params,max_iter,eps_sq,rel_prec,N,f,f32)   solver/rg_mixed_cg_her_nd.c:189-341 with
 * f = Qtm_pm_ndpsi, f32 = Qtm_pm_ndpsi_32 (op must be TMHIP_ND_OP_QTM_PM: the clover doublet has no fp32 twin and is refused) and
 * delta = solver_params.mcg_delta, on fp64 EO fields.  Zero start; fp32 inner loops with float scalars (non-pipelined, Fletcher-Reeves)
 * until the iterated residual has dropped by delta, then P += x and the true residual in fp64; fp64 inner loops once
 * iter_out >= N_outer - 2.  *iters = the reference's return value, iter_out + iter_in_sp + iter_in_dp or -1; the three counts are
 * returned as well (each pointer may be NULL).  Sums over the two flavours are added before the scalar step; fp32 sums accumulate in
 * double and are then rounded. */
int tmhip_rg_mixed_cg_her_nd(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                             int rel_prec, int N, int op, double delta, int *iters, int *iter_out, int *iter_in_sp, int *iter_in_dp);
/* mixed_cg_mms_tm_nd(Pup,Pdn,Qup,Qdn,solver_params)   solver/mixed_cg_mms_tm_nd.c:69-511 with M_ndpsi = Qtm_pm_ndpsi, M_ndpsi32 =
 * Qtm_pm_ndpsi_32 (op must be TMHIP_ND_OP_QTM_PM: the clover doublet has no fp32 twin and is refused), on fp64 EO fields, unsplit
 * lattices, 1 <= nshifts <= 32.  The arguments are those of tmhip_cg_mms_tm_nd_op.  |Q|^2 < 1e-4: what tmhip_cg_mms_tm_nd_op returns,
 * same bits (:110-113).  Otherwise every P[s] is zeroed (:264-267) and the loop of :276-462 runs in fp32 on the device: Qtm_pm_ndpsi_32
 * plus sigma_0, alpha, r and |r|^2, the stopping test (:307; the reference leaves the loop BEFORE the x update of that iteration, and
 * so does this), the zita / alpha recurrences, the reliable-update decision (:326-334, rel_delta = 1e-10), x_s += alpha_s d_s, the
 * betas, d_s = beta_s d_s + zita_s r.  Scalars are doubles, rounded to float where the reference casts them; fp32 sums accumulate in
 * double and are then rounded to float.  A reliable update (:364-442) is done by the host after its poll: P[s] += x_s, x_d += x_0,
 * r_d = Q - (A + sigma_0) x_d in fp64, the "got larger" exit for shift 0, x = 0, r = (float) r_d, new betas and d.  Every tenth
 * iteration the last active shift leaves when alpha^2 |d|^2 <= eps_sq on the updated d (:445-459) and its x is added to its P; at
 * the end the remaining x_s are added (:466-475).  *iters = the iteration j that met the precision, or -1 after max_iter iterations;
 * *rel_updates, *removed (each may be NULL) = reliable updates done, shifts removed; tmhip_nd_active_shifts reports what is left.
 * One host poll per "cg_batch" iterations; the result does not depend on it, nor on "mms32_fused". */
int tmhip_mixed_cg_mms_tm_nd(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts, int nshifts,
                             int max_iter, double eps_sq, int rel_prec, int op, int *iters, int *rel_updates, int *removed);
/* sw_deriv_nd(ieo)   operator/clover_deriv.c:156-243: swp += (1+T) sw_inv_nd summed over the chiralities, swm += their difference */
int tmhip_sw_deriv_nd(tmhip_ctx *ctx, int ieo);
/* The monomial of type NDCLOVERRAT (monomial/ndrat_monomial.c): the bodies of tmhip_ndrat_* with Qsw_pm_ndpsi, Qsw_tau1_sub_const_ndpsi and
 * H_eo_sw_ndpsi, plus the clover part of the force: tmhip_swpm_zero, four sw_spinor_eo per shift (:164-175), sw_deriv_nd(EE) when trlog
 * is set (:179-181), tmhip_sw_all(kappa, c_sw) (:182-184).  The arguments are those of tmhip_ndrat_*.  The clover term must come from
 * tmhip_sw_term, which keeps the links sw_all walks; after tmhip_set_clover the four calls refuse before any launch. */
int tmhip_ndcloverrat_force(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev,
                            double kappa, double c_sw, int trlog);
int tmhip_ndcloverrat_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, double invmaxev,
                                 double kappa, double c_sw, int trlog, int max_iter, double eps_sq, int rel_prec, int *iters);
int tmhip_ndcloverrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *nu, const double *rnu, int np, double invmaxev,
                               int max_iter, double eps_sq, int rel_prec, double *energy0, int *iters);
int tmhip_ndcloverrat_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, int max_iter,
                          double eps_sq, int rel_prec, double *energy1, int *iters);

/* ---- single-flavour multi-shift CG (solver/cg_mms_tm.c:65-197) ------------------------------------------------------------
 * cg_mms_tm(P,Q,solver_params,&reached_prec) with M_psi = Qtm_pm_psi / Qsw_pm_psi on N = VOLUME/2 sites (op TMHIP_OP_QTM_PM /
 * TMHIP_OP_QSW_PM, EO fields) or Q_pm_psi on N = VOLUME sites (op TMHIP_OP_Q_PM_FULL, FULL fields; g_mu as set by tmhip_set_mu).
 * P[s] solves (M_psi + shifts[s]^2) P = Q for s = 0 .. nshifts-1, 1 <= nshifts <= 32: shifts[0]^2 is added to the operator of the
 * CG (:88,115-118), the others are relative to it (:91); every P[s] starts at zero (any content is ignored, :85,94), Q is not
 * modified.  The last active shift is dropped every 20 iterations once alphas^2 |ps|^2 <= eps_sq (:146-153).  Stopping test
 * (:170-176): rel_prec == 0 err <= eps_sq, rel_prec > 0 err <= eps_sq |Q|^2, rel_prec < 0 none.  *iters = the reference's return
 * value: -1 when the loop ended at iteration max_iter - 1, converged there or not, else the iteration count (:193-194);
 * *reached_prec (may be NULL) = the last err (:175).  Device-resident, unsplit lattices only: a T-split context or its loopback
 * rehearsal is refused, as are nshifts outside [1, 32] and an N that does not match op. */
int tmhip_cg_mms_tm(tmhip_ctx *ctx, tmhip_field **P, tmhip_field *Q, const double *shifts, int nshifts, int max_iter, double eps_sq,
                    int rel_prec, int N, int op, int *iters, double *reached_prec);
/* shifts still active at the end of the last tmhip_cg_mms_tm (the reference's local `no_shifts`, cg_mms_tm.c:67,148) */
int tmhip_mms_active_shifts(tmhip_ctx *ctx);
/* form the last tmhip_cg_mms_tm took: 0 fused e/o stencils (cg_her's fusable shapes), 1 unfused e/o (operator, then separate
 * reductions), 2 the FULL composite Q_pm_psi; -1 before the first solve */
int tmhip_mms_form(tmhip_ctx *ctx);

/* ---- fermion force, hopping part (deriv_Sb.c:401-700) ------------------------------
 * deriv_Sb(ieo, l, k, hf, factor) accumulates 2 factor trlambda(...) of the one-hop terms into hf->derivative.  Here the
 * accumulator is device-resident: zero it, call tmhip_deriv_Sb any number of times (one call per deriv_Sb call of the
 * reference, same ieo / l / k / factor), then fetch it in the host layout su3adj df[VOLUME][4] (8 doubles per link,
 * lexicographic sites), either overwriting or adding to the host array.  T-split ranks exchange the t=0 slices of both fields with the ring
 * neighbour first (xchange_2fields, deriv_Sb.c:102); tmhip_multi_deriv_Sb is the single-process ring of n contexts. */
int tmhip_derivative_zero(tmhip_ctx *ctx);
int tmhip_deriv_Sb(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k, double factor);
int tmhip_derivative_download(tmhip_ctx *ctx, void *df, int accumulate);
int tmhip_multi_deriv_Sb(int n, tmhip_ctx **ctxs, int ieo, tmhip_field **l, tmhip_field **k, double factor);

/* sum_j deriv_Sb(ieo, l[j], k[j], hf, factor[j]) for j = 0 .. n-1, 1 <= n <= 64, added to the same accumulator (created and zeroed if
 * absent) in ONE kernel launch: the links are read and the derivative is written once, whatever n is.  The fields are only read; one field
 * may appear in several pairs and on both sides.  fp64 one-parity fields of one stride, unsplit lattices only (a T-split context and the
 * loopback rehearsal are refused); every refusal happens before the launch and leaves the accumulator untouched.  The sum over j is formed
 * before the projection onto the generators: the result differs from n tmhip_deriv_Sb calls by rounding. */
int tmhip_deriv_Sb_batch(tmhip_ctx *ctx, int ieo, int n, tmhip_field **l, tmhip_field **k, const double *factor);

/* ---- rational monomials (monomial/rat_monomial.c type RAT, monomial/ndrat_monomial.c type NDRAT) ---------------------------------
 * The three bodies of each monomial with the shifted solutions resident in HBM.  fp64 one-parity fields, unsplit lattices only (a T-split
 * context or its loopback rehearsal is refused).  mu / rmu / nu / rnu: the np entries (1 <= np <= 32) of the monomial's rational
 * approximation (rational_t::mu, rmu, nu, rnu); max_iter, eps_sq, rel_prec and *iters as in tmhip_cg_mms_tm_nd / tmhip_cg_mms_tm, which do
 * the solves into fields the context owns.  ndrat reads g_mubar, g_epsbar and the solver's phmc_invmaxev from tmhip_set_nd; `invmaxev` is
 * the monomial's EVMaxInv that the reference passes to Q_tau1_sub_const_ndpsi and uses as forcefactor (the same number in a run).
 * rat runs at twisted mass 0 as the reference sets g_mu = 0 (rat_monomial.c:62,156,222); the context's mu is back on return, errors included.
 *   *_force       the loop over the shifts given the solutions (ndrat_monomial.c:114-160, forcefactor = invmaxev; rat_monomial.c:95-132,
 *                 forcefactor = 1), ADDED to the derivative accumulator of tmhip_deriv_Sb: work fields for groups of "rat_batch" shifts
 *                 (tmhip_set_option), then two tmhip_deriv_Sb_batch launches per group
 *   *_derivative  solve, then the force (ndrat_monomial.c:96-160, rat_monomial.c:83-132)
 *   *_heatbath    pf (and pf_dn) hold the Gaussian field on entry and C eta on exit; *energy0 = |eta|^2 (:212-254, rat :175-199)
 *   *_acc         *energy1 = pf . (pf + sum_j rmu_j chi_j) (:281-309, rat :232-250); the caller forms energy1 - energy0 */
int tmhip_ndrat_force(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev);
int tmhip_ndrat_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, double invmaxev,
                           int max_iter, double eps_sq, int rel_prec, int *iters);
int tmhip_ndrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *nu, const double *rnu, int np, double invmaxev,
                         int max_iter, double eps_sq, int rel_prec, double *energy0, int *iters);
int tmhip_ndrat_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, int max_iter,
                    double eps_sq, int rel_prec, double *energy1, int *iters);
int tmhip_rat_force(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np);
int tmhip_rat_derivative(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                         int *iters);
int tmhip_rat_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *nu, const double *rnu, int np, int max_iter, double eps_sq, int rel_prec,
                       double *energy0, int *iters);
int tmhip_rat_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                  double *energy1, int *iters);
/* Type CLOVERRAT of monomial/rat_monomial.c:56-262: the rat bodies on Qsw_pm_psi / Qsw_plus_psi / H_eo_sw_inv_psi(.., 0.) at twisted mass 0
 * (mu and mu3 of the context are back on return), plus the clover part of the force: tmhip_swpm_zero, per group of "rat_batch" shifts one
 * tmhip_sw_spinor_eo_batch launch per parity (EE (w2, w3), OO (w0, chi_j); the per-call kernel with "rat_batch" 1), tmhip_sw_deriv(EE, 0.) when
 * trlog is set, tmhip_sw_all(NULL, kappa, c_sw).  The caller has run tmhip_sw_term and tmhip_sw_invert(EE, 0.) on the current links
 * (rat_monomial.c:76-78,165-166,227-228).  The context remembers parity and mu of the last tmhip_sw_invert; the four calls refuse, before any
 * launch and with every output untouched, when sw_inv is not valid, is not that of (EE, 0.) (made for OO or with mu != 0, or uploaded with
 * tmhip_set_clover), when the clover term did not come from tmhip_sw_term, on a T-split or loopback context, for np outside [1, 32] and for
 * fields that are not fp64 one-parity. */
int tmhip_cloverrat_force(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np, double kappa, double c_sw, int trlog);
int tmhip_cloverrat_derivative(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, double kappa, double c_sw, int trlog,
                               int max_iter, double eps_sq, int rel_prec, int *iters);
int tmhip_cloverrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *nu, const double *rnu, int np, int max_iter, double eps_sq, int rel_prec,
                             double *energy0, int *iters);
int tmhip_cloverrat_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                        double *energy1, int *iters);

/* ---- correction monomials (monomial/ratcor_monomial.c types RATCOR / CLOVERRATCOR, monomial/ndratcor_monomial.c types NDRATCOR /
 * NDCLOVERRATCOR) -----------------------------------------------------------------------------------------------------------------
 * fp64 one-parity fields of this context, unsplit lattices only: a T-split context or its loopback rehearsal, fp32 or FULL fields and np
 * outside [1, 32] are refused with a message, before any launch.  The two streams first:
 *   tmhip_rat_sum[_nd]     out = c (in + rmu_{np-1} chi_{np-1} + ... + rmu_0 chi_0) in ONE launch for one flavour or both, added in that order
 *                          (ratcor_monomial.c:192-196): the bits of tmhip_assign, np tmhip_assign_add_mul_r and, for c != 1, tmhip_mul_r
 *                          (:205, c = A^2).  out may be in; out may not be a chi_j.
 *   tmhip_diff_sqnorm[_nd] k = k - l and *out = |k_up|^2 (+ |k_dn|^2) in one launch and one synchronisation (:211-212,
 *                          ndratcor_monomial.c:238-240): the bits of tmhip_diff and tmhip_square_norm (their sum for two flavours),
 *                          the same bits from call to call.  Rank-local (a context that sums over ranks is refused).
 * tmhip_apply_Z / tmhip_apply_Z_nd: k = Z l = (Q^2 (A R)^2 - 1) l with R phi = phi + sum_j rmu_j (Q^2 + mu_j^2)^-1 phi, the statements of
 * ratcor_monomial.c:183-218 / ndratcor_monomial.c:202-245: solve, R, solve, R, times A^2, Q^2, minus l, norm.  op = TMHIP_OP_QTM_PM /
 * TMHIP_OP_QSW_PM (Qtm_pm_psi / Qsw_pm_psi), for _nd TMHIP_ND_OP_QTM_PM / TMHIP_ND_OP_QSW_PM (Qtm_pm_ndpsi / Qsw_pm_ndpsi); the solves are
 * tmhip_cg_mms_tm / tmhip_cg_mms_tm_nd_op with max_iter, eps_sq, rel_prec, into fields the context owns (those of the rat monomials).
 * *delta = |k|^2, *iters = the first solve's return value (what mnl->iter0 accumulates).  They run with the context's mu / mu3 as they are;
 * k may not be l.  Option "ratcor_fused" (tmhip_set_option) 1 (default): tmhip_rat_sum per application of R, the second with c = A^2, and
 * tmhip_diff_sqnorm; 0: the reference's call sequence on the single entry points.  Both give the same bits.
 * The four bodies, op as above (the clover types are the same functions with the clover operator):
 *   *_heatbath  ratcor_monomial.c:85-110 / ndratcor_monomial.c:88-123 without the random numbers: pf (and pf_dn) hold the Gaussian field eta on
 *               entry and B eta on exit, *energy0 = |eta|^2
 *   *_acc       :151-168 / :166-187: *energy1 = pf . (1 + sum_i c_i Z^i) pf; the caller forms energy1 - energy0
 * with the reference's coefficient tables, its up0 / up1 swap and its break rule.  accprec is both the solver's eps_sq and the stopping
 * threshold of the series, as in the reference (:90,106).  *napp = applications of Z, *iters = the sum of their first solves' return
 * values.  The single-flavour bodies run at twisted mass 0 (mu = mu3 = 0, :67-68,131-132), the doublet bodies with mu3 = 0 (:73,144); the
 * context's values are back on every path out, errors included.
 * The reference's loops run to i < 8 over coefs[6]: its seventh application of Z reads past the table.  These bodies apply Z at most SIX times;
 * if delta >= accprec after the sixth they fail with a message that names delta and accprec.
 * Clover types: the clover term is the caller's, as for tmhip_cloverrat_* / tmhip_ndcloverrat_*: tmhip_sw_term and tmhip_sw_invert(EE, 0.)
 * (ratcor_monomial.c:75-76,137-138), respectively tmhip_sw_term and tmhip_sw_invert_nd(mubar^2 - epsbar^2) (ndratcor_monomial.c:77-78,146-147),
 * on the current links before the call; a missing or foreign clover term is refused exactly as those functions refuse it.
 * Not built: check_C_psi / check_C_ndpsi, fp32 fields, T-split lattices (phmc_compute_ev: tmhip_eigenvalues_nd). */
int tmhip_rat_sum(tmhip_ctx *ctx, tmhip_field *out, tmhip_field *in, tmhip_field *const *chi, const double *rmu, int np, double c);
int tmhip_rat_sum_nd(tmhip_ctx *ctx, tmhip_field *out_up, tmhip_field *out_dn, tmhip_field *in_up, tmhip_field *in_dn, tmhip_field *const *chi_up,
                     tmhip_field *const *chi_dn, const double *rmu, int np, double c);
int tmhip_diff_sqnorm(tmhip_ctx *ctx, tmhip_field *k, tmhip_field *l, double *out);
int tmhip_diff_sqnorm_nd(tmhip_ctx *ctx, tmhip_field *k_up, tmhip_field *k_dn, tmhip_field *l_up, tmhip_field *l_dn, double *out);
int tmhip_apply_Z(tmhip_ctx *ctx, tmhip_field *k, tmhip_field *l, const double *mu, const double *rmu, double A, int np, int max_iter, double eps_sq,
                  int rel_prec, int op, double *delta, int *iters);
int tmhip_apply_Z_nd(tmhip_ctx *ctx, tmhip_field *k_up, tmhip_field *k_dn, tmhip_field *l_up, tmhip_field *l_dn, const double *mu, const double *rmu, double A,
                     int np, int max_iter, double eps_sq, int rel_prec, int op, double *delta, int *iters);
int tmhip_ratcor_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, double A, int np, int max_iter, double accprec, int rel_prec,
                          int op, double *energy0, int *napp, int *iters);
int tmhip_ratcor_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, double A, int np, int max_iter, double accprec, int rel_prec, int op,
                     double *energy1, int *napp, int *iters);
int tmhip_ndratcor_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, double A, int np, int max_iter,
                            double accprec, int rel_prec, int op, double *energy0, int *napp, int *iters);
int tmhip_ndratcor_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, double A, int np, int max_iter,
                       double accprec, int rel_prec, int op, double *energy1, int *napp, int *iters);

/* ---- polynomial monomial (monomial/ndpoly_monomial.c type NDPOLY, Ptilde_nd.c) ----------------------------------------------------
 * The PHMC monomial of the Wilson twisted-mass doublet, branch g_epsbar != 0 || phmc_exact_poly == 0 of its three bodies.  fp64 one-parity
 * fields of this context, unsplit lattices only.  n = MDPolyDegree (polynomial degree + 1), roots = the 2n - 2 complex MDPolyRoots as
 * (re, im) pairs, Cpol = sqrt(MDPolyLocNormConst), invmaxev = EVMaxInv.  Q_tau1_sub_const_ndpsi takes invmaxev from the argument, Qtm_ndpsi /
 * Qtm_dagger_ndpsi / Qtm_pm_ndpsi inside the bodies from tmhip_set_nd: the three bodies refuse, before any launch, an invmaxev that is not
 * the one of tmhip_set_nd.
 * Not built: type NDCLOVER (cloverndpoly), the phmc_exact_poly == 1 branches (P_ndpsi, Qtau1_P_ndpsi, Qtm_pm_sub_const_nrm_psi, Ptm_pm_psi),
 * Qtm_pm_ndbipsi, fp32 twins, T-split ranks (the eigenvalue measurement is tmhip_eigenvalues_nd); degree_of_polynomial_nd / degree_of_Ptilde and the Chebyshev
 * coefficient routines are host scalar code and stay the reference's. */
/* assign_mul_add_mul_add_mul_add_mul_r(R,S,U,V,c1,c2,c3,c4,VOLUME/2): R = c1 R + c2 S + c3 U + c4 V in that order; the fields may alias */
int tmhip_assign_mul_add_mul_add_mul_add_mul_r(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, tmhip_field *V, double c1, double c2,
                                               double c3, double c4);
/* the same kernel as the monomial uses it: out = c1 A + c2 B + c3 C + c4 D for both flavours of a doublet in one launch; out_s may be any of
 * A_s .. D_s and out_c any of A_c .. D_c; an output that is an input of the OTHER flavour is refused (other blocks of the launch read it) */
int tmhip_comb4_ndpsi(tmhip_ctx *ctx, tmhip_field *out_s, tmhip_field *out_c, tmhip_field *A_s, tmhip_field *A_c, tmhip_field *B_s, tmhip_field *B_c,
                      tmhip_field *C_s, tmhip_field *C_c, tmhip_field *D_s, tmhip_field *D_c, double c1, double c2, double c3, double c4);
/* Ptilde_ndpsi(R_s,R_c,dd,n,S_s,S_c,Qsq)   Ptilde_nd.c:102-203: Clenshaw's recursion over the n Chebyshev coefficients on [evmin, evmax]
 * (phmc_cheb_evmin / phmc_cheb_evmax), Qsq = op (TMHIP_ND_OP_QTM_PM or TMHIP_ND_OP_QSW_PM, the latter with a valid sw_inv_nd).  The copies of
 * the reference are a rotation of three work doublets the context owns: a step is one Qsq and one launch of the four-term kernel.  S is not
 * modified, R may be S flavour by flavour (R_s = S_s, R_c = S_c; R_s = S_c or R_c = S_s is refused).  n < 1 is refused. */
int tmhip_Ptilde_ndpsi(tmhip_ctx *ctx, tmhip_field *R_s, tmhip_field *R_c, const double *coefs, int n, tmhip_field *S_s, tmhip_field *S_c, double evmin,
                       double evmax, int op);
/* ndpoly_derivative   ndpoly_monomial.c:79-117, ADDED to the accumulator of tmhip_deriv_Sb with forcefactor = -Cpol invmaxev.  pf is only read.
 * The ascending chain chi[1 .. n-2] stays in HBM (2 (n - 2) fields; chi[0] is pf).  The descending loop runs in groups of G = "poly_batch"
 * steps (tmhip_set_option): 6 G + 2 work fields per group (G + 1 running chi_hi doublets, the H_eo_tm_ndpsi of chi[j-1] and of chi_hi per
 * step) and ONE tmhip_deriv_Sb_batch launch per parity with 2 G pairs; "poly_batch" 1 is the reference's call order on tmhip_deriv_Sb.
 * Work fields that a call with a smaller G or n no longer needs are freed at its start.
 * Refused before the first launch, the accumulator untouched: a failed allocation (the force then frees all of its work fields, so a retry
 * with a smaller "poly_batch" starts from nothing), n < 3, a T-split context or its loopback rehearsal, fp32 / FULL fields or fields of
 * another stride, no gauge field, an invmaxev other than that of tmhip_set_nd. */
int tmhip_ndpoly_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev);
/* ndpoly_heatbath   :179-209, 255-256 without the RANLUX lines and phmc_compute_ev (the caller's, as for tmhip_ndrat_heatbath; tmhip_eigenvalues_nd measures it): pf holds
 * the Gaussian field on entry and Ptilde B^dagger Q eta on exit, *energy0 = |eta|^2; the chain ping-pongs between two doublets */
int tmhip_ndpoly_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev,
                          const double *ptilde_coefs, int ptilde_n, double evmin, double evmax, double *energy0);
/* ndpoly_acc   :282-368: the chain, Ener[0] = |B pf|^2, then up to seven correction steps in the reference's alternating order with its
 * binomial bookkeeping and its stop rule |Ener[j] - Ener[j-1]| < precision_hfinal; *energy1 = Ener at the index the reference ends with,
 * *corrections = steps taken (1 .. 7).  md_coefs: the n MDPolyCoefs.  ener (may be NULL): Ener[0 .. 7], zero beyond the last step taken. */
int tmhip_ndpoly_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev,
                     const double *md_coefs, const double *ptilde_coefs, int ptilde_n, double evmin, double evmax, double precision_hfinal,
                     double *energy1, int *corrections, double *ener /* 8 */);

/* Clover part of the force (monomial/cloverdet_monomial.c:110-147): the insertion matrices swm / swp (clover_leaf.c:141) are
 * device-resident; zero them, accumulate the spinor outer products (operator/clover_deriv.c:252) and the tr-log term
 * (clover_deriv.c:72; needs sw_inv of that parity), then tmhip_sw_all (operator/clover_accumulate_deriv.c:58) adds the sixteen
 * link derivatives per plane and site to the SAME derivative accumulator tmhip_deriv_Sb uses.  gauge_field = NULL reuses the
 * lexicographic copy kept by the last tmhip_sw_term.  tmhip_get_swpm returns su3 swm[VOLUME][4] / swp[VOLUME][4].
 * T-split ranks: sw_spinor_eo / sw_deriv are site-local; sw_all exchanges its contributions to the neighbours' links (see below). */
int tmhip_swpm_zero(tmhip_ctx *ctx);
int tmhip_sw_spinor_eo(tmhip_ctx *ctx, int ieo, tmhip_field *kk, tmhip_field *ll, double fac);
int tmhip_sw_deriv(tmhip_ctx *ctx, int ieo, double mu);
/* sum_j sw_spinor_eo(ieo, kk[j], ll[j], fac[j]) for j = 0 .. n-1, 1 <= n <= 64, in ONE launch: swm / swp of parity ieo are read and written
 * once, whatever n is.  The fields are only read; one field may appear in several pairs.  fp64 one-parity fields of one stride; site-local,
 * so T-split contexts are served.  The sum over j is formed before it is added: the result differs from n calls by rounding. */
int tmhip_sw_spinor_eo_batch(tmhip_ctx *ctx, int ieo, int n, tmhip_field **kk, tmhip_field **ll, const double *fac);
int tmhip_sw_all(tmhip_ctx *ctx, const void *gauge_field, double kappa, double c_sw);
/* sw_all on a T-split lattice held by n contexts of THIS process (peer copies instead of RCCL for the two-sided derivative halo
 * that xchange/xchange_deri.c ships); every context needs its own tmhip_sw_term (which keeps the links incl. halo slabs). */
int tmhip_multi_sw_all(int n, tmhip_ctx **ctxs, double kappa, double c_sw);
int tmhip_get_swpm(tmhip_ctx *ctx, void *swm, void *swp);

/* ---- clover twisted mass (invert_clover_eo.c:63-165) ------
 * The 6x6 site blocks are inputs like the gauge field: `sw` = su3 sw[VOLUME][3][2] from sw_term
 * (operator/clover_term.c:88), `sw_inv` = su3 sw_inv[VOLUME][4][2] from sw_invert(EE, mu)
 * (operator/clover_invert.c:170; +mu set in [0,V/2), -mu set in [V/2,V)).  Call again whenever they change. */
int tmhip_set_clover(tmhip_ctx *ctx, const void *sw, const void *sw_inv);
/* ... or computed on the device: sw_term(gf, kappa, c_sw) (operator/clover_term.c:88) from the host gauge field handed
 * over exactly as for tmhip_set_gauge, then sw_invert(ieo, mu) (operator/clover_invert.c:170; the operators below expect
 * ieo = 0 = EE as operator.c:364 uses it).  tmhip_get_clover copies the blocks back in the reference's host layouts
 * (either pointer may be NULL) for host code that still wants them. */
int tmhip_sw_term(tmhip_ctx *ctx, const void *gauge_field, double kappa, double c_sw);
int tmhip_sw_invert(tmhip_ctx *ctx, int ieo, double mu);
int tmhip_get_clover(tmhip_ctx *ctx, void *sw, void *sw_inv);
/* The tr-log energies on the device's sw (operator/clover_det.c:115 sw_trace, :202 sw_trace_nd), sites of parity ieo:
 *   sw_trace     sum_x sum_i log |det(1 + T_i(x) + i mu)|^2               (clover_trlog_monomial.c, the trlog option of cloverdet)
 *   sw_trace_nd  sum_x log( Re det_0 Re det_1 ), det_i = det((1 + T_i(x))^2 + mu^2 - eps^2)   (clovernd_trlog_monomial.c)
 * by a fully unrolled Householder triangularisation (six_det) per site and the library's fixed-order sum: the same lattice gives the same
 * bits on every run (the reference's Kahan sum over the sites is not reproduced: the values agree to rounding on the scale of
 * sum_x |term|).  Site-local, so T-split contexts are served; global != 0 adds the ranks' shares (the reference's MPI_Allreduce).
 * Refused when sw is not that of the current links (tmhip_sw_term / tmhip_set_clover after the last link update).
 * tmhip_sw_trace_failures: pivots below the reference's tiny_t met by the last of the two calls (six_det's ifail, which it only prints). */
int tmhip_sw_trace(tmhip_ctx *ctx, int ieo, double mu, int global, double *out);
int tmhip_sw_trace_nd(tmhip_ctx *ctx, int ieo, double mu, double eps, int global, double *out);
int tmhip_sw_trace_failures(tmhip_ctx *ctx);
int tmhip_clover_inv(tmhip_ctx *ctx, tmhip_field *l, int tau3sign, double mu);                                   /* clovertm_operators.c:287 */
int tmhip_clover_gamma5(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k, tmhip_field *j, double mu);     /* :448 */
int tmhip_clover(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k, tmhip_field *j, double mu);            /* :535 */
int tmhip_H_eo_sw_inv_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, int ieo, int tau3sign, double mu);     /* :268 */
int tmhip_Qsw_pm_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);                                            /* :233 */
int tmhip_Msw_plus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);                                          /* :256 */
int tmhip_Qsw_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);        /* :201  Q-hat with mu = 0 in the diagonal term */
int tmhip_Qsw_plus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);   /* :217 */
int tmhip_Qsw_minus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);  /* :209; l may alias k (invert_clover_eo.c:128) */
int tmhip_Qsw_sq_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);     /* :225 */
int tmhip_Msw_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);        /* :247 */
int tmhip_Msw_minus_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);  /* :261 */
int tmhip_Msw_full(tmhip_ctx *ctx, tmhip_field *Even_new, tmhip_field *Odd_new, tmhip_field *Even, tmhip_field *Odd);  /* :96-110 */
/* k = (1 + T + i mu g5) l on parity ieo / k = sw_inv l   (operator/assign_mul_one_sw_pm_imu_inv_block_body.c:1-72, 143-196) */
int tmhip_assign_mul_one_sw_pm_imu(tmhip_ctx *ctx, int ieo, tmhip_field *k, tmhip_field *l, double mu);
int tmhip_assign_mul_one_sw_pm_imu_inv(tmhip_ctx *ctx, int ieo, tmhip_field *k, tmhip_field *l, double mu);
int tmhip_Qsw_pm_psi_32(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);                                         /* clovertm_operators_32.c */

/* ---- mixed precision -------------------------------------
 * fp32 one-parity fields hold the reference's `spinor32` (su3.h:65-68); the fp32 gauge copy is built
 * on first use from the links given to tmhip_set_gauge. */
int tmhip_field_alloc32(tmhip_ctx *ctx, tmhip_field **out);
int tmhip_field_upload32(tmhip_ctx *ctx, tmhip_field *f, const void *host_spinor32, int nsites);
int tmhip_field_download32(tmhip_ctx *ctx, tmhip_field *f, void *host_spinor32, int nsites);
int tmhip_assign_to_32(tmhip_ctx *ctx, tmhip_field *R32, tmhip_field *S64, int N);          /* linalg/assign_to_32.c */
int tmhip_assign_to_64(tmhip_ctx *ctx, tmhip_field *R64, tmhip_field *S32, int N);          /* linalg/assign_to_64.c */
int tmhip_add_from_32(tmhip_ctx *ctx, tmhip_field *P64, tmhip_field *X32, int N);           /* assign_to_64 + add, mixed_cg_her.c:158-159 */
int tmhip_hopping_matrix_32(tmhip_ctx *ctx, int ieo, tmhip_field *l, tmhip_field *k);       /* operator/Hopping_Matrix_32.c:97-127 */
int tmhip_Qtm_pm_psi_32(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k);                    /* operator/tm_operators_32.c Qtm_pm_psi_32 */
int tmhip_square_norm_32(tmhip_ctx *ctx, tmhip_field *P, int N, int parallel, double *out);
int tmhip_scalar_prod_r_32(tmhip_ctx *ctx, tmhip_field *S, tmhip_field *R, int N, int parallel, double *out);
int tmhip_assign_add_mul_r_32(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, float c, int N);
int tmhip_assign_mul_add_r_32(tmhip_ctx *ctx, tmhip_field *R, float c, tmhip_field *S, int N);
/* l = zc (.) k [- j] on HOST spinor32 arrays of any length N (zc = z on spin 0,1, conj(z) on spin 2,3; j may be NULL; l may alias
 * k or j): the fp32 instances mul_one_pm_imu_inv_32 / assign_mul_one_pm_imu_inv_32 / mul_one_pm_imu_sub_mul_32 that
 * operator/tm_operators.c:8-47 generates and solver/Msap.c calls on domain blocks.  Staged through the device, synchronous. */
int tmhip_diag32_host(tmhip_ctx *ctx, void *l, const void *k, const void *j, double zre, double zim, int N);
/* mixed_cg_her(P,Q,params,max_iter,eps_sq,rel_prec,N,f,f32)  solver/mixed_cg_her.c:65-202 with f = Qtm_pm_psi,
 * f32 = Qtm_pm_psi_32; innereps / max_inner_it are the reference's mixcg_innereps / mixcg_maxinnersolverit
 * (default_input_values.h:193-194: 5.0e-5, 5000).  *iters = the reference's return value (-1: not converged). */
int tmhip_mixed_cg_her(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, int max_iter, double eps_sq, int rel_prec, int N,
                       int op, double innereps, int max_inner_it, int *iters, int *outer_iters);
/* Restart points of the last tmhip_mixed_cg_her: inner_iters[i] = the reference's j of outer iteration i
 * (mixed_cg_her.c:152), at most `cap` of them; *n_outer = number of outer iterations run. */
int tmhip_mixed_cg_restarts(tmhip_ctx *ctx, int *inner_iters, int cap, int *n_outer);
/* solver/rg_mixed_cg_her.c:180-347: fp32 CG with reliable updates (restart when the iterated residual fell by `delta`
 * relative to its maximum since the last update) and an fp64 fail-safe.  *iters = iter_out + iter_in_sp + iter_in_dp
 * as the reference returns it, or -1; the three counters are reported separately when the pointers are non-NULL. */
int tmhip_rg_mixed_cg_her(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, int max_iter, double eps_sq, int rel_prec, int N,
                          int op, double delta, int *iters, int *iter_out, int *iter_in_sp, int *iter_in_dp);

/* ---- molecular-dynamics updates with the links resident in HBM -------------------------------------
 * tmhip_set_gauge keeps the lexicographic links it received on the device; per MD step the links are then updated in place
 * (update_gauge.c:51-110: U <- restoresu3(exposu3(step * P)) U), the halo slabs of a T-split rank are refreshed from the
 * ring neighbours (xchange_gauge) and the stencil's gauge copy is re-sorted (update_backward_gauge.c:185-242) without any
 * host <-> device copy of the gauge field.  Momenta: su3adj [VOLUME][4] = double [VOLUME][4][8] (hamiltonian_field_t::momenta).
 * After tmhip_update_gauge the clover blocks are stale: tmhip_sw_term(ctx, NULL, ...) recomputes them from the resident links. */
int tmhip_momenta_upload(tmhip_ctx *ctx, const void *host_momenta);
int tmhip_momenta_download(tmhip_ctx *ctx, void *host_momenta);
int tmhip_update_momenta(tmhip_ctx *ctx, double step);   /* update_momenta.c:67-72 from the device-resident derivative field */
int tmhip_update_gauge(tmhip_ctx *ctx, double step);     /* update_gauge.c:51-110 */
int tmhip_multi_update_gauge(int n, tmhip_ctx **ctxs, double step);   /* the same for n contexts of one process holding a T-split lattice (peer copies) */
int tmhip_gauge_download(tmhip_ctx *ctx, void *host_gauge);   /* [VOLUMEPLUSRAND][4] su3, e.g. at the end of a trajectory */

/* ---- the frame of a trajectory around the integrator (update_tm.c, monomial/moment_energy.c, monomial/monitor_forces.c) --------
 * fp64, on the resident links, momenta and derivative; nothing crosses the bus but the scalars.
 * The snapshot is the reference's gauge_tmp: a device buffer of its own in the layout of the resident links (own sites and, on a
 * T-split rank, the two halo slabs), allocated by the first tmhip_gauge_snapshot (576 bytes per site) and freed by
 * tmhip_gauge_snapshot_free or tmhip_destroy; tmhip_set_gauge leaves it alone.  _snapshot without resident links, _restore and
 * _snapshot_diff without a snapshot return non-zero with a message.
 * tmhip_gauge_restore and tmhip_gauge_reunitarize change the links and leave every derived state as tmhip_update_gauge leaves it
 * (stencil gauge copy, fp32 and packed twins stale, "gauge_recon" 12 guard re-run, clover blocks stale); the flow buffers and the
 * snapshot are not touched.  _reunitarize is ONE pass: links read, restoresu3 (expo.c:118-137), written back and scattered into the
 * stencil's copy.  restoresu3 is a function of the single link, so a T-split rank reunitarises its halo slabs itself and no exchange
 * follows; the snapshot holds the slabs, so _restore needs none either.
 * The three sums are over the rank's own links (with the option "gauge_global_sums" 1 over all ranks of a T split; the maximum is
 * then the maximum over the ranks); fixed-order block sums, two calls on the same data return the same bits.  They do not reproduce
 * the order of the reference's serial Kahan loops: every term is non-negative and the result lies within a few dozen ulp of the exact
 * sum (tests/test_gpu_trajectory_frame.py derives the bound from the launch geometry).
 * tmhip_derivative_norms returns non-zero if no force has created the derivative field yet. */
int tmhip_gauge_snapshot(tmhip_ctx *ctx);                   /* update_tm.c:109-121  gauge_tmp <- links */
int tmhip_gauge_restore(tmhip_ctx *ctx);                    /* update_tm.c:329-339  links <- gauge_tmp (reject) */
int tmhip_gauge_snapshot_free(tmhip_ctx *ctx);
int tmhip_gauge_reunitarize(tmhip_ctx *ctx);                /* update_tm.c:313-328  restoresu3_in_place on every link (accept) */
int tmhip_gauge_snapshot_diff(tmhip_ctx *ctx, double *out); /* update_tm.c:233-272  sum over own links of sqrt(|U - U_tmp|_F^2) */
int tmhip_moment_energy(tmhip_ctx *ctx, double *out);       /* moment_energy.c:46-74 0.5 * sum over own links of |P|^2 */
int tmhip_derivative_norms(tmhip_ctx *ctx, double *sum, double *max);   /* monitor_forces.c:64-89 over own links: sum and maximum of d1^2 + ... + d8^2 */
/* device time per call (HIP events over reps calls) of one form of the reject / accept pass, for tools/traj_speed.py: form 0 restore as copy +
 * re-sort, 1 restore in one pass, 2 accept as a restoresu3 pass + re-sort, 3 accept in one pass.  Needs resident links and a snapshot;
 * leaves the links restored (0, 1) or reunitarised (2, 3). */
int tmhip_bench_trajectory_forms(tmhip_ctx *ctx, int form, int reps, double *ms);
/* whole-field copies across the bus this context has made so far: out[0] tmhip_set_gauge, [1] tmhip_gauge_download, [2] tmhip_momenta_upload,
 * [3] tmhip_momenta_download -- what a test of "nothing crosses the bus between the snapshot and the acceptance step" reads */
int tmhip_transfer_counts(tmhip_ctx *ctx, long long out[4]);
/* su3adj df[VOLUME][4] (host) -> the device derivative field, replacing what it holds: the inverse of tmhip_derivative_download(..., 0) */
int tmhip_derivative_upload(tmhip_ctx *ctx, const void *df);

/* ---- gauge monomial on the device-resident links (monomial/gauge_monomial.c; gauge.hip) --------------------------------
 * tmhip_gauge_derivative ADDS gauge_derivative (glambda = 0) / gauge_EMderivative of the reference to the derivative accumulator of
 * tmhip_deriv_Sb / tmhip_sw_all (created and zeroed if no force has done so yet): for every link factor trlambda(U staple^dagger) with
 * the plaquette staples (get_staples.c; planes with direction 0 weighted 1 + glambda, spatial planes 1 - glambda) and, with
 * use_rectangles, the rectangle staples (get_rectangle_staples.c) weighted factor c1 / c0; factor = -c0 beta / 3 with rectangles,
 * -beta / 3 without.  The three measures return this rank's share (sites of the local VOLUME) of measure_plaquette /
 * measure_gauge_action / measure_rectangles, i.e. the value before the reference's MPI_Allreduce (option "gauge_global_sums" 1: after it).  All four need the resident links
 * (tmhip_set_gauge); two calls on the same links give bit-identical results.  T-split ranks (nproc_t > 1): the plaquette force and sums
 * use the one-deep halo slabs tmhip_update_gauge keeps current; rectangles reach two slices deep and return non-zero there. */
int tmhip_gauge_derivative(tmhip_ctx *ctx, double beta, double c0, double c1, int use_rectangles, double glambda);
int tmhip_measure_plaquette(tmhip_ctx *ctx, double *out);
int tmhip_measure_gauge_action(tmhip_ctx *ctx, double glambda, double *out);
int tmhip_measure_rectangles(tmhip_ctx *ctx, double *out);

/* ---- Wilson gradient flow and clover field strength on the device-resident links (meas/gradient_flow.c,
 *      meas/measure_clover_field_strength_observables.c; flow.hip) -------------------------------------------------------
 * fp64, unsplit lattices.  The flow works on private copies: the resident links, the stencil's gauge copy and the clover blocks are
 * never touched.  tmhip_flow_begin allocates two link buffers and Z (2 x 576 + 288 bytes per site) and copies the resident links in
 * (calling it again restarts from the links resident then); tmhip_flow_step is one step_gradient_flow (third-order Runge-Kutta,
 * plaquette staples, cayley_hamilton_exponent); tmhip_flow_observables returns P = measure_plaquette / (6 VOLUME) and E, Q of
 * measure_clover_field_strength_observables on the flowed links; tmhip_flow_end frees the buffers (tmhip_destroy does so too).
 * tmhip_gradient_flow is the loop of gradient_flow_measurement: it measures at t = 0, then takes pairs of steps while (t[1] < tmax)
 * with t[step] = t[step-1] + eps, and writes one row of eight doubles per pair at the odd step,
 *   t  P  Eplaq = 36 (1 - P)  Esym  t^2 Eplaq  t^2 Esym  Wsym = t^2 (2 E_1 + t (E_2 - E_0) / (2 eps))  Qsym,
 * at most max_rows of them (non-zero, nothing written past them, if the loop needs more); *nrows = rows written.
 * Two calls on the same links give bit-identical results.  All return non-zero, launching nothing, without resident links
 * (tmhip_set_gauge) and on a T-split rank (nproc_t > 1: the link halo would have to be refreshed after every stage);
 * _step / _observables / _download also without a preceding tmhip_flow_begin. */
int tmhip_measure_field_strength(tmhip_ctx *ctx, double *E, double *Q);      /* on the resident links */
int tmhip_flow_begin(tmhip_ctx *ctx);
int tmhip_flow_step(tmhip_ctx *ctx, double eps);
int tmhip_flow_observables(tmhip_ctx *ctx, double *P, double *E, double *Q);
int tmhip_flow_download(tmhip_ctx *ctx, void *host_gauge);                   /* flowed links, [VOLUME][4] su3 */
int tmhip_flow_end(tmhip_ctx *ctx);
int tmhip_gradient_flow(tmhip_ctx *ctx, double eps, double tmax, int max_rows, double *rows, int *nrows);

/* ---- the other online measurements (meas/correlators.c, meas/pion_norm.c, meas/polyakov_loop.c, meas/oriented_plaquettes.c; meas.hip)
 * fp64.  Each call is one kernel, one final pass over its partial sums and ONE synchronisation, however many numbers it returns; the
 * sums are added in a fixed order without atomics, so two calls on the same data give bit-identical results.
 * tmhip_slice_correlators: the raw per-slice sums of a propagator given as its two one-parity halves (TMHIP_FIELD_EO, fp64), both
 *   parities added: pp[s] = sum psi^+ psi, pa[s] = sum Re psi^+ (gamma0 psi), p4[s] = sum Im psi^+ (gamma5 gamma0 psi), composed from
 *   _gamma0, _gamma5, _spinor_prod_re, _spinor_prod_im as correlators.c:165-169 does.  dir 0: time-slices, T values per array
 *   (correlators.c:159-170); dir 3: z-slices, LZ values (pion_norm.c:98-107); any other dir returns non-zero.  pa and p4 may be NULL
 *   (pion_norm needs pp only; with both NULL the bilinear is not computed).  Normalisation, the sign of pa, 1 / (2 kappa^2) and the output file stay with the caller.  The sum
 *   is site-local: a T-split rank (nproc_t > 1) gets its local T slices (dir 0) or its share of every z-slice (dir 3) and the caller
 *   adds over the ranks as the reference's MPI_Reduce does.  fp32 fields, FULL fields and fields of another context return non-zero
 *   with a message and launch nothing.
 * tmhip_polyakov_loop: the trace of the ordered product of the L_dir links along dir = 0 .. 3 from coordinate 0, summed over the
 *   VOLUME / L_dir lines and divided by 3 VOLUME / L_dir (polyakov_loop.c:366-392, :498-537), on the resident links (tmhip_set_gauge,
 *   kept current by tmhip_update_gauge).  An extent below 3 along dir returns non-zero (the reference's loop multiplies three links
 *   there), as do a T-split rank and a context without resident links.
 * tmhip_measure_oriented_plaquettes: the averages of Re tr P_{mu nu} / 3 over the sites for the planes (0,1), (0,2), (0,3), (1,2),
 *   (1,3), (2,3), each divided by VOLUME (oriented_plaquettes.c:52-78); their sum times 3 VOLUME is tmhip_measure_plaquette.  Resident
 *   links, unsplit lattices. */
int tmhip_slice_correlators(tmhip_ctx *ctx, const tmhip_field *even, const tmhip_field *odd, int dir, double *pp, double *pa, double *p4);
int tmhip_polyakov_loop(tmhip_ctx *ctx, int dir, double *re, double *im);
int tmhip_measure_oriented_plaquettes(tmhip_ctx *ctx, double plaq[6]);

/* ---- ILDG gauge configurations (io/gauge_read.c:28-198, io/gauge_read_binary.c:140-200, io/gauge_write.c:22-59,
 *      io/gauge_write_binary.c:150-175, io/dml.c:49-60).  The "ildg-binary-data" record travels to / from the device as it lies in
 *      the file; byte swap, 32 <-> 64 bit conversion, site and link re-ordering and the SciDAC checksum happen in HBM (ildg.hip). -- */
typedef struct {
  int gauge_read;                       /* GaugeInfo.gaugeRead */
  unsigned suma, sumb;                  /* checksum calculated over the record (GaugeInfo.checksum) */
  unsigned suma_stored, sumb_stored;    /* ... and as stored in the "scidac-checksum" record */
  int prec, lx, ly, lz, lt;             /* "ildg-format" record */
  char xlf_info[1024];                  /* GaugeInfo.xlfInfo */
  char ildg_data_lfn[512];              /* GaugeInfo.ildg_data_lfn */
} tmhip_gauge_info;
/* this rank's part of the record (T LZ LY LX sites, x fastest; per site links x, y, z, t; big-endian; prec 64 | 32) -> resident links +
 * stencil gauge copy as after tmhip_set_gauge; sums[2] = SciDAC checksum A, B of this rank's sites (XOR over ranks = the file's) */
int tmhip_gauge_unpack_ildg(tmhip_ctx *ctx, const void *file_bytes, int prec, unsigned *sums);
int tmhip_gauge_pack_ildg(tmhip_ctx *ctx, void *file_bytes, int prec, unsigned *sums);
/* read_gauge_field(filename, gf) / write_gauge_field(filename, prec, xlfInfo), LIME framing included (both also on T-split ranks, collective:
 * every rank reads / writes its contiguous part of the record at its offset, the checksum is combined over the ranks, rank 0 writes the
 * framing records -- the file is byte for byte the one a single rank writes); the reader returns 0
 * or -1 with the reference's messages (io_checks = !g_disable_IO_checks; prec_expected = gauge_precision_read_flag);
 * host_gauge (may be NULL): the host's g_gauge_field to fill as well; xlf_info: the formatted "xlf-info" message or NULL */
int tmhip_read_gauge_field(tmhip_ctx *ctx, const char *filename, int prec_expected, int io_checks, void *host_gauge, tmhip_gauge_info *info);
int tmhip_write_gauge_field(tmhip_ctx *ctx, const char *filename, int prec, const char *xlf_info, unsigned *sums);

/* ---- propagators and sources (io/spinor_read.c, io/spinor_write.c, io/spinor_read_binary.c, io/spinor_write_binary.c, start.c).  The
 *      "scidac-binary-data" record travels to / from the device as it lies in the file; parity selection, the x <-> z transposition
 *      between the e/o fields and the file's site order, byte swap, 32 <-> 64 bit conversion and the SciDAC checksum happen in HBM
 *      (spinor_io.hip). -- */
/* io/spinor_write_binary.c:145-224 (write_binary_spinor_data) and io/spinor_read_binary.c (read_binary_spinor_data) with
 * io/dml.c:49-60: this rank's contiguous part of the record (host pointer; T LZ LY LX sites, x fastest; per site the 24 reals of
 * `spinor`, su3.h:60-63, big-endian; prec 64 | 32 with the (float) cast / exact widening of io/utils.h) from / into two fp64 EO
 * fields: file site (t, x, y, z) is entry g_lexic2eosub[g_ipt[t][x][y][z]] of `even` if (t_global + x + y + z) % 2 == 0, else of
 * `odd`.  sums[2] = SciDAC checksum A, B of this rank's sites with rank = proc_t T LZ LY LX + site number (XOR over the ranks of a
 * T split = the file's, io/dml.c:63-66).  Entries [VOLUME/2, stride) of the planes are not written.  The `_l` forms of the
 * reference (write_binary_spinor_data_l / read_binary_spinor_data_l: one lexicographic field) are these same calls on a FULL field
 * passed as tmhip_field_even(full), tmhip_field_odd(full). */
int tmhip_spinor_pack(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, void *file_bytes, int prec, unsigned *sums);
int tmhip_spinor_unpack(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, const void *file_bytes, int prec, unsigned *sums);
typedef struct {
  int prec;                             /* 64 | 32, from the length of the record (spinor_read.c:83-95) */
  int prop_type;                        /* parse_propagator_type after the switch of spinor_read.c:40-55: 0, 1 or 10 */
  int position;                         /* the "scidac-binary-data" record that was read (2 position + 1 for Source_Sink_Pairs) */
  int checksum_read;                    /* a "scidac-checksum" record followed and parsed (always 0 with io_checks = 0) */
  unsigned suma, sumb;                  /* calculated over the record */
  unsigned suma_stored, sumb_stored;    /* as stored in the file */
} tmhip_spinor_info;
/* io/spinor_read.c:27-150 read_spinor(s, r, filename, position) with io/utils_parse_propagator_type.c:22-91, unsplit lattices only
 * (fails with a message on a T-split context).  Returns 0, or with the reference's messages on stderr: -2 / -3 propagator / source
 * types that are not supported, -5 no such "scidac-binary-data" record, -6 a record of the wrong length, -1 no "scidac-checksum"
 * record behind the data (io_checks = g_disable_src_IO_checks != 1), -7 the data could not be read; 1 for errors the reference does
 * not return from (no such file, no device memory).  Calculated and stored checksum are NOT compared, as in the reference, which
 * only prints them: both are in `info` (may be NULL).  Unlike the reference, -1 is found before the data are touched: a refused
 * file leaves the fields as they were. */
int tmhip_read_spinor(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, const char *filename, int position, int io_checks, tmhip_spinor_info *info);
/* io/spinor_write.c:23-47 write_spinor(writer, s, r, flavours, prec): per flavour a "scidac-binary-data" header (MB 1, ME 0), the record
 * packed on the device, and the "scidac-checksum" message (0, 1; io/utils_write_checksum.c:30-44).  append = 0 creates the file,
 * 1 adds to it.  sums (may be NULL): 2 words per flavour.  Unsplit lattices only. */
int tmhip_write_spinor(tmhip_ctx *ctx, const char *filename, int append, tmhip_field *const *even, tmhip_field *const *odd, int flavours, int prec, unsigned *sums);
/* write_header + write_message + close_writer_record (io/utils.h) for the records around the data ("propagator-type", "inversion-info",
 * "etmc-propagator-format", "source-type", "etmc-source-format"): the text is the caller's, as with "xlf-info" on the gauge side */
int tmhip_write_lime_message(const char *filename, int append, const char *type, const char *text, int mb, int me);
/* start.c:707-741 source_spinor_field(P, Q, is, ic) (global_site 0) and start.c:743-830 source_spinor_field_point_from_file(P, Q, is, ic,
 * source_indx): both fields zero, component (is, ic) = 1.0 at the site whose GLOBAL index is global_site = ((t LX + x) LY + y) LZ + z --
 * z fastest --, on the rank and in the field (even: P, odd: Q) that own it */
int tmhip_source_point(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, int is, int ic, long long global_site);

/* ---- multi-GPU halo exchange (replaces xchange_field / xchange_halffield,
 *      xchange/xchange_field.c:269-470, xchange/xchange_halffield.c:176-263) -- */
#define TMHIP_UNIQUE_ID_BYTES 128
int tmhip_comm_get_unique_id(char id[TMHIP_UNIQUE_ID_BYTES]);             /* rank 0, then broadcast by the host program */
int tmhip_comm_init(tmhip_ctx *ctx, const char id[TMHIP_UNIQUE_ID_BYTES]); /* ring of nproc_t ranks along T over RCCL */
/* The same ring WITHOUT RCCL: the ranks of a node meet in a POSIX shared-memory segment named after `job` (1 .. 64 characters, the same
 * string on every rank of the job, different between jobs -- e.g. the launcher's job id), and faces, halo slices and scalar sums travel
 * device -> page-locked host memory -> that segment -> device, stream-ordered on the compute stream with no overlap: the reference's own
 * MPI exchange on host memory (xchange/xchange_field.c:98-250, linalg/square_norm.c:299-316).  Not the fast path; it needs nothing but
 * the node's memory and lets several ranks share one GPU (how the multi-rank code is tested as real processes on a one-GPU box).
 * Collective over the ranks; replaces tmhip_comm_init for this context.  Sums are added in rank order: the same bits on every rank. */
int tmhip_comm_init_shm(tmhip_ctx *ctx, const char *job);
/* The direct face carrier, on top of either ring (collective, after tmhip_comm_init / tmhip_comm_init_shm): every rank maps its two
 * neighbours' receive buffers (hipIpcGetMemHandle / hipIpcOpenMemHandle; the handles travel over the communicator the context has) and
 * the kernels that produce the projected half-spinor faces store them straight into the neighbour's memory -- over xGMI between GPUs,
 * through the mapping between processes that share a GPU.  It replaces the MPI_Isend / MPI_Irecv / MPI_Waitall of
 * xchange/xchange_halffield.c:176-263 (operator/halfspinor_body.c:281-317) for the faces; sums and the other halos stay on the
 * communicator.  No copy, no kernel of a communication library, nothing on the receiver's compute units; on lattices whose boundary
 * waves fit the wait budget a stencil of a T-split rank is ONE kernel ("direct_form").  Non-zero (and the faces stay on the communicator,
 * on EVERY rank) when some rank cannot map a neighbour.  A single rank behind the one-rank RCCL communicator of
 * tmhip_comm_set_loopback(ctx, 2) may call it too: the collective set-up runs over RCCL with np = 1 and the rank becomes its own
 * neighbour (the single-GPU rehearsal of this function and of the direct sums). */
int tmhip_comm_init_ipc(tmhip_ctx *ctx);
/* 1 when the faces travel as direct stores (0: over the communicator); *sharers (may be NULL): ranks of the job on this rank's GPU */
int tmhip_comm_faces_direct(tmhip_ctx *ctx, int *sharers);
/* 1 when the scalar sums over the ranks travel as direct stores too (option "direct_sums", every rank's block mapped by every rank):
 * MPI_Allreduce of linalg/square_norm.c:314 as ONE wave per rank, added in rank order (the same bits on every rank) */
int tmhip_comm_sums_direct(tmhip_ctx *ctx);
/* tmhip_comm_init builds TWO communicators over the same ranks: one for the half-spinor faces (second HIP stream), one
 * (ncclCommSplit of the first) for the scalar all-reduces of the linalg (MPI_Allreduce in linalg/square_norm.c:314) and the
 * force halos on the main stream.  Ranks in each as RCCL reports them (ncclCommCount); 0, 0 before tmhip_comm_init. */
int tmhip_comm_count(tmhip_ctx *ctx, int *nranks_faces, int *nranks_reduce);
/* 1: the reductions have their own communicator; 0: ncclCommSplit was unavailable (or switched off with the "comm_split" option) and
 * they share the face communicator -- still correct, a face exchange is never in flight together with a reduction; -1: no communicator */
int tmhip_comm_is_split(tmhip_ctx *ctx);
/* Single-GPU self-test of the split-phase path: faces are packed, "exchanged"
 * with this rank itself and consumed by the exterior kernel.  on = 1: device-to-device
 * copies; on = 2: through a one-rank RCCL communicator (ncclSend/ncclRecv to self); on = 3: the direct carrier onto
 * oneself (the neighbours' receive buffers are this rank's own). */
int tmhip_comm_set_loopback(tmhip_ctx *ctx, int on);
/* Test hook: holds the comm stream back for `ms` milliseconds (<= 20000) in front of the next thing enqueued on it, i.e. the next halo
 * exchange -- what a late neighbour looks like from this rank (xchange_field's MPI_Waitall simply waits, xchange/xchange_field.c:98-250;
 * so does the split path here, up to "flag_timeout_ms").  Changes no result. */
int tmhip_comm_stream_delay_ms(tmhip_ctx *ctx, int ms);

/* Single-process ring of n contexts (ctxs[r] = rank r of an n-way T split; one per GPU, or several
 * on one GPU as a self-test): Hopping_Matrix on every slab with the faces moved by peer copies
 * (hipMemcpyPeerAsync) instead of RCCL.  Same pack / stencil / exterior kernels as the RCCL path. */
int tmhip_multi_hopping_matrix(int n, tmhip_ctx **ctxs, int ieo, tmhip_field **l, tmhip_field **k);

/* ---- measurement ---------------------------------------------------------- */
/* The benchmark.c:291-300 loop on device-resident fields: iters x {H(0,f1,f0); H(1,f2,f1)},
 * timed with HIP events on the context's stream.  ms_total = elapsed milliseconds. */
int tmhip_bench_hopping(tmhip_ctx *ctx, tmhip_field *f0, tmhip_field *f1, tmhip_field *f2, int iters, double *ms_total);
/* `reps` launches of the spinor record's pack (pack != 0) or unpack kernel alone, timed with HIP events: no host copy, no checksum
 * fetch.  The record is the one a first pack of (even, odd) leaves in the staging buffer; an unpack rewrites the fields with their
 * own values (at 32 bit: rounded). */
int tmhip_bench_spinor_io(tmhip_ctx *ctx, tmhip_field *even, tmhip_field *odd, int prec, int pack, int reps, double *ms_total);
/* generic event slots (0..15) recorded on the context's compute stream */
int tmhip_event_record(tmhip_ctx *ctx, int slot);
int tmhip_event_elapsed_ms(tmhip_ctx *ctx, int slot_start, int slot_stop, double *ms);
/* Launch-shape and scheduling options; the defaults are the measured best.  Apart from "gauge_recon" (below) none of
 * them changes a result beyond rounding (reduction order, FMA contraction); unknown names are refused.
 * TMLQCD_HIP_OPTIONS="name=value,name=value" in the environment applies them when the context is created (executables linked against
 * the drop-in unmodified); a malformed or unknown entry fails tmhip_create.
 *   "block" 0|256|64 threads per block (0: automatic, 64 on local lattices of fewer than 131072 sites per parity)
 *   "xcd"   block order: 2 automatic (default; tile order up to L = 32, slab order above -- and on lattices of fewer than 24 time-slices
 *           whose time-slices are large (L >= 24): one rank's share of a T split, profiles/r04_shape_sweep.log), 0 none, 1 one chunk per XCD,
 *           3 slab, 4 tile;  "tgrp" time-slices per tile group (0 = automatic)
 *   "occ" / "occ32"  waves per SIMD allowed by a dynamic-LDS cap for the fp64 / fp32 stencil (3 / 0 = no cap)
 *   "minw" 4: __launch_bounds__(BS, 4)
 *   "split_sync" 0 (default) | 1: T-split ranks -- 0: the exterior kernel (main stream) and the pack kernel (comm stream) wait on the device for a
 *                flag of the other stream; 1: the two streams are ordered by HIP events, no wait on the device at all (slower: two events on the
 *                main stream per stencil)
 *                ("split_pipe" of round 3 is gone: slower than the default form since the stencil kernel has one store path, and the direct carrier
 *                does what it was for -- faces of a chain's next stencil on their way while the current one runs -- without an RCCL kernel;
 *                profiles/r04_split_forms.md)
 *   "direct_form" -1 (default) | 0 | 1: the direct carrier (tmhip_comm_init_ipc) -- 1: one kernel per stencil (the boundary waves wait for their
 *                neighbour's word after their seven local hops, add the hop across the cut, project their output and store the projection into the
 *                neighbour's buffer); 0: stencil kernel + exterior kernel (which waits and pushes); -1: one kernel while the boundary waves of a
 *                launch are at most 2048 (fp64 clover epilogues: 1792; ranks sharing a GPU in a rehearsal: 1024 / their number)
 *   "direct_sums" 1 (default) | 0 (before tmhip_comm_init_ipc): with the direct carrier every rank maps every rank's block and the scalar sums
 *                over the ranks (square_norm .. with parallel = 1, the alpha and the stopping test of cg_her) are one wave that stores this
 *                rank's partial sum into every rank's block and adds up its own row in rank order (the same bits on every rank) instead
 *                of an ncclAllReduce
 *   "direct_order" bit 0 / bit 1: one-kernel form -- boundary time-slices dispatched first (else last) in a stencil whose faces are packed now /
 *                were pushed ahead by the stencil before (default 3: first in both; with the slab order of short lattices the boundary slices are
 *                spread over all XCDs and going first is worth 2 - 3 % at T_local 8 / 16, profiles/r04_split_forms_ab.log)
 *   "prepack" 1 (default) | 0: T-split ranks -- the exterior kernel also projects the completed boundary slices of its output into the send buffers, so
 *                the next stencil of a chain (Qtm_pm_psi, a fused CG iteration) starts its exchange without a pack kernel
 *   "flag_timeout_ms" bound of those device-side waits (default 120 s, or TMLQCD_HIP_FLAG_TIMEOUT_S in the environment; 0 = none): a late
 *                neighbour is waited for, a dead one becomes an error of the next synchronising call (reported once, then cleared)
 *   "comm_split" 1|0 (before tmhip_comm_init / tmhip_comm_set_loopback(2)): 0 keeps the reductions on the face communicator (the fallback of an RCCL without ncclCommSplit)
 *   "cg_fused_dot" 2 (default: alpha / residual / norm in the stencil epilogues), 1 scalar product only, 0 plain linalg kernels
 *   "cg_self" 1 (default) | 0: small unsplit lattices (the hop-split stencil) -- the fused CG iteration adds up its partial sums inside the residual stencil
 *                (alpha) and the (P, p) kernel (stopping test, beta) instead of two one-block sum + scalar kernels in between
 *   "nd_fused" 1 (default) | 0: the doublet operators (tmhip_*_ndpsi, the nd solvers) -- 1: one stencil per hop for both flavours with the
 *                flavour mixing in its epilogue; 0: two single-flavour stencils per hop and a mixing pass.  It sets
 *                the form of the fp32 doublet (tmhip_Qtm_pm_ndpsi_32, the inner loops of tmhip_rg_mixed_cg_her_nd) as well, whose default
 *                is the faster form at 32^4 of profiles/r20_nd32_speed.log: 1
 *   "mms32_fused" 1 (default) | 0: the vector part of an iteration of tmhip_mixed_cg_mms_tm_nd after the shift-0 residual kernel and the
 *                one-block beta kernel -- 1: ONE pass over all shifts and both flavours that reads x_s, d_s and the shared r and writes x_s and
 *                d_s (four field passes of 96 B/site per shift and flavour); 0: the fp64 solver's shape, an x pass and a d pass (six).  The same
 *                element operations in the same order: identical bits.  Default: the faster form at 32^4 of profiles/r21_mixed_mms_speed.log
 *   "nd_mms_mixed" 0 (default) | 1: 1 routes the multi-shift solves of the Wilson twisted-mass doublet monomials (tmhip_ndrat_derivative /
 *                _heatbath / _acc, tmhip_apply_Z_nd and the ndratcor calls with TMHIP_ND_OP_QTM_PM) through tmhip_mixed_cg_mms_tm_nd, what
 *                solver_params.type == MIXEDCGMMSND does in the reference (monomial/ndrat_monomial.c:107,228,291); the clover doublet keeps
 *                tmhip_cg_mms_tm_nd_op.  0: nothing changes
 *   "rat_batch" shifts per group of the rat / ndrat force (clamped to [1, 32], default 12, the fastest of 1 / 2 / 4 / 12
 *                measured at 16^4 and 32^4 with np = 12, profiles/r08_rat_speed.log): one tmhip_deriv_Sb_batch launch per parity and group
 *                and, for the clover types (ndcloverrat, cloverrat), one tmhip_sw_spinor_eo_batch launch per parity and group; 1: the per-call
 *                tmhip_sw_spinor_eo kernel in the reference's order
 *   "poly_batch" steps of the descending loop per group of tmhip_ndpoly_derivative (clamped to [1, 32], default 12: with n = 49 the fastest
 *                of 1 / 2 / 4 / 12 / 32 at 16^4; at 32^4 32 is 2.7 % faster but holds 194 work fields instead of 74, 12 GB more,
 *                profiles/r14_poly_speed.log): one tmhip_deriv_Sb_batch launch per parity and group; 1: tmhip_deriv_Sb per pair in the
 *                reference's order
 *   "ratcor_fused" 1 (default) | 0: tmhip_apply_Z[_nd] and the bodies of the correction monomials -- 1: one tmhip_rat_sum launch per application
 *                of R (all np solutions of both flavours, A^2 folded into the second) and one tmhip_diff_sqnorm launch with one synchronisation;
 *                0: the reference's call sequence on tmhip_assign / _assign_add_mul_r / _mul_r / _diff / _square_norm.  The same bits either way.
 *   "poly_fail_alloc" k (tests only; default 0 = off): the k-th work-field allocation of the polynomial monomial from now on fails, once,
 *                the way an exhausted device makes it fail
 *   "gauge_global_sums" 0 (default) | 1: tmhip_measure_plaquette / _gauge_action / _rectangles return the rank's own share (0: the reference's value
 *                before its MPI_Allreduce) or the sum over the ranks of a T split (1: its return value; needs the communicator, like parallel = 1)
 *   "csg_batch" 1 (default) | 0: tmhip_chrono_guess on the batched kernels (tmhip_multi_scalar_prod, tmhip_multi_assign_diff_mul, tmhip_lincomb)
 *                or as a sequence of the complex singles
 *   "eig_basis" m (default 24; 3 .. TMHIP_EIG_MAX_BASIS), "eig_cheb" d (default 4; 0 = no filter), "eig_fused" 1 (default) | 0 -- the fastest
 *                measured forms at 32^4, profiles/r19_eig_speed.log: the
 *                eigenvalue measurement, tmhip_eigenvalues / tmhip_eigenvalues_nd (described there); "eig_restarts" n (default 0 = no
 *                bound): a run ends after n Lanczos cycles as it ends at max_apps (the max_iterations of the drop-in's eigenvalues_bi)
 *   "cg_sync" 1: host-side scalars as in the reference loop;  "cg_batch" n: iterations enqueued between two polls of `done`
 *   "gauge_cache" -1 (automatic) / 0 / 1: the 64-thread stencil launches of small unsplit lattices, and the stencil launches of a T-split rank,
 *                  load the links with (0) or without (1) the streaming hint; automatic = without while the gauge copy is <= 200 MB (it then
 *                  stays in the Infinity Cache between calls: 4 x 32^3 per rank 65 -> 80 % of the unsplit rate, profiles/r04_gcache_ab.log)
 *   "swall_order" 0 / 1 / 2: block order of the owner-computes sw_all (one chunk per XCD / slab order / sw_term's tile order, default: fabric reads
 *                6.6 -> 4.0 GB per launch at 32^4, 3 % faster -- the kernel is bound by its 43 dependent 3x3 products per link, not by bytes;
 *                profiles/r04_swall_ab.log)
 *   "swterm_order" 0 / 1: block order of sw_term (one chunk per XCD / small (x, y) tiles walked through all time-slices, default)
 * One option changes what is read from memory:
 * "gauge_recon" = 12 makes the twisted-mass stencil launches (fp64 and fp32) fetch only the first two rows of every link and
 * rebuild the third as conj(row0 x row1) in registers (the 12-real compression the reference exposes for its external
 * inverters, misc_types.h:29-33 COMPRESSION_12) -- 25 % fewer bytes per site.  The 12-real instances are 256-thread kernels:
 * launches with 64-thread blocks ("block" 64, or the automatic choice below 131072 sites per parity on an unsplit lattice)
 * keep the full read.  It is opt-in and guarded: the links of the resident gauge field must be SU(3) to 1e-13, otherwise the
 * option is refused with a message and the full 18-real read stays in force (set the option again to have links that are
 * SU(3) again judged anew).  The rule: no stencil, operator or solver launch reads 12 reals of links whose max |row2 -
 * conj(row0 x row1)| exceeds 1e-13.  The deviation is measured on the device when the option is set and, while it is in
 * force, again by every call that changes the links the stencil reads, before that call returns: tmhip_set_gauge, the ILDG
 * reader, tmhip_update_gauge, tmhip_multi_update_gauge, tmhip_sw_term / tmhip_sw_all with host links, tmhip_resort_gauge.
 * Molecular-dynamics updates need this: restoresu3 normalises rows 0 and 1 of exp(step P) without orthogonalising them, so
 * updated links leave SU(3) by 1e-7 after two steps with |step P| = 2.5 and by 1e-13 after some hundred ordinary ones.
 * The measurement is one launch and one synchronisation per such call; with the default 18-real read nothing is added.
 * "gauge_pack" -1 (automatic, default) | 0 | 1 changes what is read but never a result: the staged 256-thread fp64 stencil with a
 * twisted-mass epilogue on an unsplit lattice reads a packed twin of the gauge copy -- two rows of every link and a 16-byte tail: the distance of the
 * third row from its rebuild conj(row_a x row_b) as six 21-bit offsets in ulps, and two bits that say which cyclic rotation of the rows
 * was stored: 112 bytes instead of 144.  The twin is built on the context's stream by the first such launch after the links changed (one kernel, a 12-byte copy
 * and one synchronisation per change of the links) and every link is verified there bit for bit with the stencil's own rebuild
 * function; a field in which some link has no exact rotation is read in full, silently.  0: never; 1: as automatic.  "gauge_recon" 12 takes
 * precedence.  "gauge_pack_rot" -1 (default: the first rotation that verifies) | 0 | 1 | 2 (try that rotation first; for tests). */
int tmhip_set_option(tmhip_ctx *ctx, const char *name, int value);
/* the value an option has now, for a caller that changes one around a call and puts it back: "eig_basis", "eig_cheb", "eig_fused", "eig_restarts" */
int tmhip_get_option(tmhip_ctx *ctx, const char *name, int *value);
/* The packed twin of the gauge copy ("gauge_pack"), built now if it is stale: out = {1 if the stencil may read it else 0, links stored on
 * rotation 0, 1, 2, links without an exact rotation}.  tmhip_gauge_pack_build_ms: device time of the last build. */
int tmhip_gauge_pack_stats(tmhip_ctx *ctx, long long out[5]);
int tmhip_gauge_pack_build_ms(tmhip_ctx *ctx, double *ms);
/* bytes per link the stencil reads of the twin, built now if it is stale: 104 (the two kept rows in their compact form: low words as they
 * are, high words as 26-bit fields with a five-bit exponent and one escape per link -- exact, like everything else here), 112 (some link has
 * a kept real at or above 2, a subnormal, or two reals below 2^-30: the rows as plain doubles), 0 (some link has no rotation: read in full).
 * "gauge_pack_compact" -1 (default) | 1: the 104-byte form where the whole field fits it; 0: never (A/B runs, tests). */
int tmhip_gauge_pack_format(tmhip_ctx *ctx, int *bytes_per_link);
/* stencil launches of this context that read the packed copy (either form) so far */
int tmhip_gauge_pack_launches(tmhip_ctx *ctx, long long *n);
/* max |row2 - conj(row0 x row1)| over all links of the resident gauge field */
int tmhip_gauge_su3_deviation(tmhip_ctx *ctx, double *maxdev);

#ifdef __cplusplus
}
#endif
#endif
