/* tmlqcd_dropin.h -- the reference's own symbols, implemented on MI355X (libtmlqcd_dropin.so).
 *
 * Every function below has EXACTLY the name, signature and argument meaning of the
 * tmLQCD function cited next to it, so `benchmark`, `invert` and `hmc_tm` link against
 * this library instead of the corresponding objects of liboperator.a / liblinalg.a /
 * libsolver.a (link line configure.in:1074) with no source change.  Host arrays stay in
 * the reference's AoS `spinor` / `su3` layouts (su3.h:40-63).
 *
 * The library reads these tmLQCD globals AT CALL TIME (never cached across calls):
 *   T, LX, LY, LZ, VOLUME, RAND (global.h:82-84), g_nproc_t/x/y/z, g_proc_coords (global.h:206-207),
 *   g_gauge_field, g_update_gauge_copy (global.h:176,73), ka0..ka3 (boundary.h:25), g_mu (global.h:198),
 *   and -- weak references, a host program without them gets 0 / the plain branch -- g_mu3 (clover odd-odd twist,
 *   global.h:197), g_c_sw (clover branch of D_psi, global.h:198), sw / sw_inv (clovertm_operators.c:58-59),
 *   mixcg_innereps, mixcg_maxinnersolverit (read_input.h:112-113), g_prec_sequence_d_dagger_d, g_precWS, update_backward_gauge.
 *
 * Residency (SURVEY §7 "hard parts"): the reference API passes host pointers.  Two modes:
 *   COHERENT (default) every call uploads its inputs and downloads its outputs: always
 *            correct for unmodified callers, PCIe-bound.
 *   RESIDENT           outputs stay in HBM; a host array is uploaded only when it has no
 *            valid device mirror.  The host copy of an output is stale until
 *            tmlqcd_hip_sync_to_host(); after the host writes an array call
 *            tmlqcd_hip_host_modified().  cg_her() always runs device-resident
 *            internally and returns with P valid on the host.
 * Errors are fatal (print + exit), the reference's convention (fatal_error.c).
 */
#ifndef TMLQCD_DROPIN_H
#define TMLQCD_DROPIN_H
#ifdef __cplusplus
extern "C" {
#define TM_COMPLEX double _Complex
#else
#include <complex.h>
#define TM_COMPLEX double _Complex
#endif

/* su3.h:40-63 -- layout is ABI */
typedef struct { TM_COMPLEX c00, c01, c02, c10, c11, c12, c20, c21, c22; } su3;
typedef struct { TM_COMPLEX c0, c1, c2; } su3_vector;
typedef struct { su3_vector s0, s1, s2, s3; } spinor;
typedef void (*matrix_mult)(spinor *const, spinor *const); /* solver/matrix_mult_typedef.h:30 */

/* ---- stencil ------------------------------------------------------------- */
void Hopping_Matrix(const int ieo, spinor *const l, spinor *const k);        /* operator/Hopping_Matrix.h:30 */
void Hopping_Matrix_nocom(const int ieo, spinor *const l, spinor *const k);  /* operator/Hopping_Matrix_nocom.h */
void tm_times_Hopping_Matrix(const int ieo, spinor *const l, spinor *const k, TM_COMPLEX const cfactor); /* operator/tm_times_Hopping_Matrix.h */
void tm_sub_Hopping_Matrix(const int ieo, spinor *const l, spinor *p, spinor *const k, TM_COMPLEX const cfactor); /* operator/tm_sub_Hopping_Matrix.h */
void D_psi(spinor *const P, spinor *const Q);                                 /* operator/D_psi.h:27 */

/* ---- operator/tm_operators.h:26-77 ---------------------------------------- */
void Qtm_plus_psi(spinor *const l, spinor *const k);
void Qtm_plus_psi_nocom(spinor *const l, spinor *const k);
void Qtm_minus_psi(spinor *const l, spinor *const k);
void Mtm_plus_psi(spinor *const l, spinor *const k);
void Mtm_plus_psi_nocom(spinor *const l, spinor *const k);
void Mtm_minus_psi(spinor *const l, spinor *const k);
/* symmetric e/o preconditioning, operator/tm_operators.h:57-65 */
void Qtm_plus_sym_psi(spinor *const l, spinor *const k);
void Qtm_plus_sym_psi_nocom(spinor *const l, spinor *const k);
void Qtm_minus_sym_psi(spinor *const l, spinor *const k);
void Mtm_plus_sym_psi(spinor *const l, spinor *const k);
void Mtm_plus_sym_dagg_psi(spinor *const l, spinor *const k);
void Mtm_minus_sym_psi(spinor *const l, spinor *const k);
void Mtm_plus_sym_psi_nocom(spinor *const l, spinor *const k);
void Mtm_minus_sym_psi_nocom(spinor *const l, spinor *const k);
void Qtm_pm_sym_psi(spinor *const l, spinor *const k);
void Qtm_pm_psi(spinor *const l, spinor *const k);
void Qtm_pm_psi_nocom(spinor *const l, spinor *const k);
void H_eo_tm_inv_psi(spinor *const l, spinor *const k, const int ieo, const double sign);
void M_full(spinor *const Even_new, spinor *const Odd_new, spinor *const Even, spinor *const Odd);
void Q_full(spinor *const Even_new, spinor *const Odd_new, spinor *const Even, spinor *const Odd);
void M_minus_1_timesC(spinor *const Even_new, spinor *const Odd_new, spinor *const Even, spinor *const Odd);
void mul_one_pm_imu_inv(spinor *const l, const double _sign, const int N);
void assign_mul_one_pm_imu_inv(spinor *const l, spinor *const k, const double _sign, const int N);
void assign_mul_one_pm_imu(spinor *const l, spinor *const k, const double _sign, const int N);
void mul_one_pm_imu(spinor *const l, const double _sign);
void mul_one_pm_imu_sub_mul(spinor *const l, spinor *const k, spinor *const j, const double _sign, const int N);
void mul_one_pm_imu_sub_mul_gamma5(spinor *const l, spinor *const k, spinor *const j, const double _sign); /* tm_operators.c:813 */
void mul_one_sub_mul_gamma5(spinor *const l, spinor *const k, spinor *const j);                              /* tm_operators.c:781 */
void Mee_psi(spinor *const l, spinor *const k, const double mu);
void Mee_inv_psi(spinor *const l, spinor *const k, const double mu);
void Q_pm_psi(spinor *const l, spinor *const k);
void Q_plus_psi(spinor *const l, spinor *const k);
void Q_minus_psi(spinor *const l, spinor *const k);
void M_minus_psi(spinor *const l, spinor *const k);
void D_dagg_psi(spinor *const l, spinor *const k);
typedef struct { float c[24]; } spinor32;   /* su3.h:83: spinor32 = 4 x su3_vector32 = 12 complex float */
/* fp32 twins on HOST spinor32 arrays by their reference names (row f1).  Operands are copied in and results out on every call (the
 * coherent semantics; the fp32 solvers iterate device-resident through mixed_cg_her / rg_mixed_cg_her below).  N <= VOLUME/2. */
void Hopping_Matrix_32(const int ieo, spinor32 *const l, spinor32 *const k);              /* operator/Hopping_Matrix_32.h:31 */
void Hopping_Matrix_32_orphaned(const int ieo, spinor32 *const l, spinor32 *const k);     /* :30 -- called by EVERY thread of an enclosing OpenMP team: one issues the device call, all meet before and after */
void Qtm_pm_psi_32(spinor32 *const l, spinor32 *const k);                                 /* operator/tm_operators_32.c:94 */
float square_norm_32(const spinor32 *const P, const int N, const int parallel);           /* linalg/square_norm_32.c:95 */
float scalar_prod_r_32(const spinor32 *const S, const spinor32 *const R, const int N, const int parallel);   /* linalg/scalar_prod_r_32.c:109 */
void assign_add_mul_r_32(spinor32 *const R, spinor32 *const S, const float c, const int N);                  /* linalg/assign_add_mul_r_32.c:104 */
void assign_mul_add_r_32(spinor32 *const R, const float c, const spinor32 *const S, const int N);            /* linalg/assign_mul_add_r_32.c:81 */
void diff_32(spinor32 *const Q, const spinor32 *const R, const spinor32 *const S, const int N);              /* linalg/diff_32.c:39 */
void assign_to_32(spinor32 *const R, spinor *const S, const int N);                       /* linalg/assign_to_32.c:37 */
void assign_to_64(spinor *const R, spinor32 *const S, const int N);                       /* linalg/assign_to_32.c:84 (N = VOLUME/2) */
void mul_one_pm_imu_inv_32(spinor32 *const l, const double _sign, const int N);                                        /* tm_operators.c:74 */
void assign_mul_one_pm_imu_inv_32(spinor32 *const l, spinor32 *const k, const double _sign, const int N);              /* tm_operators.h */
void mul_one_pm_imu_sub_mul_32(spinor32 *const l, spinor32 *const k, spinor32 *const j, const double _sign, const int N); /* tm_operators.c:103 */
void Q_pm_psi_prec(spinor *const l, spinor *const k);   /* tm_operators.c:402; spinorPrecondition stays reference code (weak reference) */
void Q_pm_psi2(spinor *const l, spinor *const k);       /* tm_operators.c:453 */
void Q_pm_psi_gpu(spinor *const l, spinor *const k);    /* tm_operators.c:440; gamma5 is applied to k IN PLACE first */
void Q_minus_psi_gpu(spinor *const l, spinor *const k); /* tm_operators.c:476; likewise */
void Q_psi(spinor *const P, spinor *const Q);
void gamma5(spinor *const l, spinor *const k, const int V);                   /* gamma.h */

void tmlqcd_hip_comm_init(const char unique_id[128]); /* ranks along T: id from tmhip_comm_get_unique_id, broadcast (MPI_Bcast) by the host */
void tmlqcd_hip_comm_init_shm(const char *job);         /* the same ring without RCCL: host-staged through a shared-memory segment of the node (tmhip_comm_init_shm) */
int tmlqcd_hip_comm_init_ipc(void);                      /* after either: the half-spinor faces travel as direct stores into the ring neighbours' IPC-mapped receive buffers
                                                          * (tmhip_comm_init_ipc; replaces the MPI_Isend/Irecv/Waitall of xchange/xchange_halffield.c:176-263).  Collective.
                                                          * Non-zero when some rank cannot map a neighbour: every rank then keeps the communicator's exchange */
double square_norm(const spinor *const P, const int N, const int parallel);
double scalar_prod_r(const spinor *const S, const spinor *const R, const int N, const int parallel);
void assign_add_mul_r(spinor *const P, spinor *const Q, const double c, const int N);
void assign_add_mul(spinor *const P, spinor *const Q, const _Complex double c, const int N);                 /* linalg/assign_add_mul.h: P += c Q */
void assign_mul_add_r(spinor *const R, const double c, const spinor *const S, const int N);
double assign_mul_add_r_and_square(spinor *const R, const double c, const spinor *const S, const int N, const int parallel);
void diff(spinor *const Q, const spinor *const R, const spinor *const S, const int N);
void assign(spinor *const R, spinor *const S, const int N);
void add(spinor *const Q, const spinor *const R, const spinor *const S, const int N);   /* linalg/add.h */
void mul_r(spinor *const R, const double c, spinor *const S, const int N);               /* linalg/mul_r.h */
_Complex double scalar_prod(const spinor *const S, const spinor *const R, const int N, const int parallel);   /* linalg/scalar_prod.h: sum conj(S) R */
void assign_diff_mul(spinor *const S, spinor *const R, const _Complex double c, const int N);                /* linalg/assign_diff_mul.h: S -= c R */
void mul(spinor *const R, const _Complex double c, spinor *const S, const int N);                            /* linalg/mul.h: R = c S, R may be S */
void assign_add_mul_add_mul(spinor *const R, spinor *const S, spinor *const U, const _Complex double c1, const _Complex double c2,
                            const int N);                                                                    /* linalg/assign_add_mul_add_mul.h: R += c1 S + c2 U */
void assign_mul_bra_add_mul_ket_add(spinor *const R, spinor *const S, spinor *const U, const _Complex double c1, const _Complex double c2,
                                    const int N);                                                            /* linalg/assign_mul_bra_add_mul_ket_add.h: R = c2 (R + c1 S) + U */

/* ---- solver/cg_her.h ------------------------------------------------------- */
int cg_her(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec,
           const int N, matrix_mult f);

/* ---- solver/bicgstab_complex.h -----------------------------------------------
 * P is the starting guess and receives the solution; returns the iteration count, or -1 after max_iter iterations or on a breakdown.
 * f = Qtm_plus_psi, Qtm_minus_psi, Mtm_plus_psi, Mtm_minus_psi, Mtm_plus_sym_psi, Mtm_minus_sym_psi, Qsw_plus_psi, Qsw_minus_psi or
 * Msw_plus_psi with N = VOLUME/2, or D_psi (g_c_sw <= 0) with N = VOLUME, on an unsplit lattice: the whole solve runs on the device
 * (tmhip_bicgstab_complex).  Any other f, N or a T-split run: the reference's loop over the drop-in linalg, one call at a time in
 * coherent mode, f called through host pointers. */
int bicgstab_complex(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec,
                     const int N, matrix_mult f);

/* ---- solver/chrono_guess.h: the chronological guess of the det / cloverdet / detratio / cloverdetratio monomials -----------
 * chrono_guess: trial = the Galerkin solution of f x = phi in the span of the _n stored vectors v[index_array[0 .. _n-1]]; the stored
 * vectors older than the newest one are orthogonalised against it in place.  _N <= 0, or _n = 0 (an empty list: the reference reads
 * index_array[-1] there), gives trial = 0; _N > 20 ends the program with a message (the reference's buffers hold 20).  f from the
 * table of cg_her runs on the device with the batched kernels (option csg_batch); any other f is called through host pointers, the
 * linalg around it one call at a time in coherent mode.  Returns 0.
 * chrono_add_solution: stores trial / |trial| in the list and advances index_array and *_n as the reference does. */
int chrono_guess(spinor *const trial, spinor *const phi, spinor **const v, int index_array[], const int _N, const int _n, const int V,
                 matrix_mult f);
void chrono_add_solution(spinor *const trial, spinor **const v, int index_array[], const int _N, int *_n, const int V);

/* ---- operator/clovertm_operators.h ----------------------- */
/* The host keeps computing `sw` / `sw_inv` with its own sw_term / sw_invert (operator.c:329-330,364); the library
 * reads the globals `su3 ***sw, ***sw_inv` (clovertm_operators.c:58-59).  They carry no dirty flag in the reference,
 * so call tmlqcd_hip_update_clover() after every sw_term / sw_invert (first use uploads automatically). */
void tmlqcd_hip_update_clover(void);
void Qsw_pm_psi(spinor *const l, spinor *const k);                                                  /* clovertm_operators.c:233 */
void Msw_plus_psi(spinor *const l, spinor *const k);                                                /* :256 */
void Qsw_psi(spinor *const l, spinor *const k);                                                     /* :201 */
void Qsw_plus_psi(spinor *const l, spinor *const k);                                                /* :217 */
void Qsw_minus_psi(spinor *const l, spinor *const k);                                               /* :209 (in place in invert_clover_eo.c:128) */
void Qsw_sq_psi(spinor *const l, spinor *const k);                                                  /* :225 */
void Msw_psi(spinor *const l, spinor *const k);                                                     /* :247 */
void Msw_minus_psi(spinor *const l, spinor *const k);                                               /* :261 */
void Msw_full(spinor *const Even_new, spinor *const Odd_new, spinor *const Even, spinor *const Odd); /* :96 */
void assign_mul_one_sw_pm_imu(const int ieo, spinor *const k, spinor *const l, const double mu);     /* assign_mul_one_sw_pm_imu_inv_block_body.c:1 */
void assign_mul_one_sw_pm_imu_inv(const int ieo, spinor *const k, spinor *const l, const double mu); /* :143 */
void Mee_sw_psi(spinor *const k, spinor *const l, const double mu);                                 /* clovertm_operators.c:873 */
void Mee_sw_inv_psi(spinor *const k, spinor *const l, const double mu);                             /* :1098 */
void H_eo_sw_inv_psi(spinor *const l, spinor *const k, const int ieo, const int tau3sign, const double mu); /* :268 */
void clover_inv(spinor *const l, const int tau3sign, const double mu);                              /* :287 */
void clover_gamma5(const int ieo, spinor *const l, const spinor *const k, const spinor *const j, const double mu); /* :448 */
void clover(const int ieo, spinor *const l, const spinor *const k, const spinor *const j, const double mu);        /* :535 */

/* ---- solver/mixed_cg_her.h ------------------------------ */
/* `solver_params_t` (solver/solver_params.h:46-109) is passed BY VALUE.  Being larger than 16 bytes it travels in
 * memory under the SysV ABI, ahead of the stack-passed `f32`, so the callee must know its exact size and the offset
 * of the one field read on this path (mcg_delta, solver_params.h:68).  The mirror below restates that layout --
 * field order and types are ABI, like `spinor` and `su3` -- with neutral names for the fields this library never
 * reads.  tests/test_gpu_link_reference_caller.py has reference code build the struct and call through it. */
typedef void (*matrix_mult32)(void *const, void *const);   /* solver/matrix_mult_typedef.h:32 */
typedef struct {
  int eigcg_i[5];                  /* eigcg_nrhs .. eigcg_ldh */
  double eigcg_d[3];               /* eigcg_tolsq1, eigcg_tolsq, eigcg_restolsq */
  int eigcg_rand_guess_opt;
  float mcg_delta;                 /* reliable-update threshold of rg_mixed_cg_her */
  int type, max_iter, rel_prec, no_shifts, sdim;
  double squared_solver_prec;
  void (*M_psi)(spinor *const, spinor *const);
  matrix_mult32 M_psi32;
  void (*M_ndpsi)(spinor *const, spinor *const, spinor *const, spinor *const);
  void (*M_ndpsi32)(void *const, void *const, void *const, void *const);
  double *shifts;
  int solution_type, compression_type, sloppy_precision, external_inverter;   /* enums, misc_types.h */
} tmlqcd_solver_params;
/* solver/mixed_cg_her.c:65-202 reads the globals mixcg_innereps / mixcg_maxinnersolverit (read_input.h:112-113),
 * not the struct. */
int mixed_cg_her(spinor *const P, spinor *const Q, tmlqcd_solver_params solver_params, const int max_iter,
                 double eps_sq, const int rel_prec, const int N, matrix_mult f, matrix_mult32 f32);
/* solver/rg_mixed_cg_her.c:180 */
int rg_mixed_cg_her(spinor *const P, spinor *const Q, tmlqcd_solver_params solver_params, const int max_iter,
                    const double eps_sq, const int rel_prec, const int N, matrix_mult f, matrix_mult32 f32);

/* ---- operator/tm_operators_nd.h, solver/cg_her_nd.h, solver/cg_mms_tm_nd.h: the non-degenerate doublet --------
 * g_mubar, g_epsbar (global.h:202) and phmc_invmaxev (phmc.h:31) are read at every call (weak references: a host program
 * without them gets 0, 0, 1).  Unsplit lattices only: with g_nproc_t > 1 every symbol below ends the program with a message.
 * The output pair may be the input pair where the reference allows it (Qtm_pm_ndpsi, M_ee_inv_ndpsi, H_eo_tm_ndpsi,
 * mul_one_pm_itau2).  Of the polynomial helpers Ptilde_ndpsi is here (with the monomial NDPOLY, further down); those of the
 * phmc_exact_poly == 1 branches (P_ndpsi, Qtau1_P_ndpsi, Qtm_pm_sub_const_nrm_psi, Ptm_pm_psi) and Qtm_pm_ndbipsi are not built.
 * The clover doublet follows below. */
typedef void (*matrix_mult_nd)(spinor *const, spinor *const, spinor *const, spinor *const);   /* solver/matrix_mult_typedef.h:33 */
void Qtm_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);          /* :68-89 */
void Qtm_dagger_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);   /* :130-152 */
void Qtm_pm_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);       /* :195-238 */
void M_ee_inv_ndpsi(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c, const double mu, const double eps);  /* :639-696 */
void H_eo_tm_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm, const int ieo);   /* :508-519 */
void mul_one_pm_itau2(spinor *const p, spinor *const q, spinor *const r, spinor *const s, const double sign, const int N);        /* :582-597 */
/* :311-380; l must not be k (the reference hops into l before it reads k) */
void Q_tau1_sub_const_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm,
                            const _Complex double z, const double Cpol, const double invev);
/* solver/cg_her_nd.c:57-160 and solver/cg_mms_tm_nd.c:64-215 run on the device for f / M_ndpsi = Qtm_pm_ndpsi or Qsw_pm_ndpsi on
 * N = VOLUME/2 sites (up to 32 shifts); anything else ends the program with a message */
int cg_her_nd(spinor *const P_up, spinor *P_dn, spinor *const Q_up, spinor *const Q_dn, const int max_iter, double eps_sq,
              const int rel_prec, const int N, matrix_mult_nd f);
int cg_mms_tm_nd(spinor **const Pup, spinor **const Pdn, spinor *const Qup, spinor *const Qdn, tmlqcd_solver_params *solver_params);
/* ---- operator/tm_operators_nd_32.c, solver/rg_mixed_cg_her_nd.h: the fp32 doublet and the mixed-precision doublet solve ----
 * The three operators act on HOST spinor32 arrays of VOLUME/2 sites like the fp32 twins above: operands are copied in and results out
 * on every call; (float) g_mubar, (float) g_epsbar and (float) phmc_invmaxev * phmc_invmaxev are read as the reference reads them.
 * The output pair may be the input pair. */
typedef void (*matrix_mult_nd32)(spinor32 *const, spinor32 *const, spinor32 *const, spinor32 *const);   /* solver/matrix_mult_typedef_nd.h:32 */
void Qtm_pm_ndpsi_32(spinor32 *const l_strange, spinor32 *const l_charm, spinor32 *const k_strange, spinor32 *const k_charm);   /* tm_operators_nd_32.c:215 */
void M_ee_inv_ndpsi_32(spinor32 *const l_s, spinor32 *const l_c, spinor32 *const k_s, spinor32 *const k_c, const float mu, const float eps);   /* :137 */
void M_oo_sub_g5_ndpsi_32(spinor32 *const l_s, spinor32 *const l_c, spinor32 *const k_s, spinor32 *const k_c, spinor32 *const j_s,
                          spinor32 *const j_c, const float mu, const float eps);                                                   /* :200 */
/* solver/rg_mixed_cg_her_nd.c:189-341, `solver_params_t` by value as for rg_mixed_cg_her above (mcg_delta is the field read).  Runs on
 * the device, with the fields resident as for cg_her_nd, for f = Qtm_pm_ndpsi on N = VOLUME/2 sites: the fp32 operator is then
 * Qtm_pm_ndpsi_32 whatever f32 is.  Anything else (Qsw_pm_ndpsi has no fp32 twin here) ends the program with a message. */
int rg_mixed_cg_her_nd(spinor *const P_up, spinor *const P_dn, spinor *const Q_up, spinor *const Q_dn, tmlqcd_solver_params solver_params,
                       const int max_iter, const double eps_sq, const int rel_prec, const int N, matrix_mult_nd f, matrix_mult_nd32 f32);
/* solver/mixed_cg_mms_tm_nd.c:69-511: the fp32 multi-shift CG with reliable updates (solver = mixedcgmmsnd, solver/monomial_solve.c:252-268).
 * Runs on the device, with the fields resident as for cg_mms_tm_nd, for M_ndpsi = Qtm_pm_ndpsi, M_ndpsi32 = Qtm_pm_ndpsi_32 and
 * sdim = VOLUME/2 (up to 32 shifts); anything else ends the program with a message, as cg_mms_tm_nd does. */
int mixed_cg_mms_tm_nd(spinor **const Pup, spinor **const Pdn, spinor *const Qup, spinor *const Qdn, tmlqcd_solver_params *solver_params);
/* ---- the clover doublet: operator/tm_operators_nd.h (Qsw_*), operator/clovertm_operators.h (the _nd functions), operator/clover_leaf.h ----
 * fp64, unsplit lattices.  The device's clover term must belong to the current links (tmlqcd_hip_sw_term, or the host's sw_term followed
 * by tmlqcd_hip_update_clover), and sw_invert_nd(mubar^2 - epsbar^2) must have run on it, as ndrat_monomial.c:89-91 does; otherwise every
 * symbol below ends the program with a message.  sw_invert_nd keeps its result on the device beside sw_inv (cloverdet's inverse is not
 * overwritten there) and copies it into the first VOLUME/2 entries of the host's sw_inv when the program has one, where the reference puts
 * it.  sw_deriv_nd adds to the device-resident swm / swp of tmlqcd_hip_swpm_zero / tmlqcd_hip_sw_all.  These two are site-local and
 * also run on T-split ranks; everything else of this block ends the program there.  A program that keeps the reference's
 * clover_invert.o / clover_deriv.o on its link line resolves these two names there, not here.
 * Order when cloverdet and the clover doublet alternate: tmlqcd_hip_sw_term, tmlqcd_hip_sw_invert(EE, mu), THEN sw_invert_nd.  A
 * degenerate clover symbol called after sw_invert_nd without tmlqcd_hip_sw_invert in between uploads the host's sw / sw_inv again --
 * whose first half now holds the doublet's inverse -- and drops sw_inv_nd.
 * tmlqcd_hip_sw_invert_failures() returns six_invert's count of near-singular pivots of the last inversion (the reference prints it).
 * Not here: the clover doublet's fp32 twin (Qsw_pm_ndpsi_32; the twisted-mass doublet's, Qtm_pm_ndpsi_32, is above), Qsw_pm_ndbipsi,
 * clover_nd. */
void sw_invert_nd(const double mshift);                                                                                  /* clover_invert.c:440 */
void sw_deriv_nd(const int ieo);                                                                                         /* clover_deriv.c:156 */
int tmlqcd_hip_sw_invert_failures(void);
/* The tr-log energies (operator/clover_det.c; replaces clover_det.o, which holds nothing else that has a caller outside it): from the
 * device's clover term where it belongs to the current links, else the host's sw is uploaded first.  Site-local: they run on T-split
 * ranks and return the sum over all ranks there, as the reference's MPI_Allreduce does.  The sum over the sites is the library's fixed-order
 * one, not the reference's Kahan sum: the same bits on every run, equal to the reference's value to rounding on the scale of sum |term|.
 * tmlqcd_hip_sw_trace_failures(): six_det's ifail of the last of the two calls, which the reference only prints. */
double sw_trace(const int ieo, const double mu);                                                                         /* clover_det.c:115 */
double sw_trace_nd(const int ieo, const double mu, const double eps);                                                    /* clover_det.c:202 */
int tmlqcd_hip_sw_trace_failures(void);
void assign_mul_one_sw_pm_imu_eps(const int ieo, spinor *const k_s, spinor *const k_c, const spinor *const l_s, const spinor *const l_c,
                                  const double mu, const double eps);                                                    /* clovertm_operators.c:960 */
void clover_inv_nd(const int ieo, spinor *const l_c, spinor *const l_s);                                                 /* :352 */
void clover_gamma5_nd(const int ieo, spinor *const l_c, spinor *const l_s, const spinor *const k_c, const spinor *const k_s,
                      const spinor *const j_c, const spinor *const j_s, const double mubar, const double epsbar);        /* :733 */
void Qsw_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);          /* tm_operators_nd.c:91-111 */
void Qsw_dagger_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);   /* :154-174 */
void Qsw_pm_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);       /* :240-285 */
void Qsw_tau1_sub_const_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm,
                              const _Complex double z, const double Cpol, const double invev);                            /* :378-444; l != k */
void H_eo_sw_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);      /* :521-535 */
void Msw_ee_inv_ndpsi(spinor *const l_strange, spinor *const l_charm, spinor *const k_strange, spinor *const k_charm);   /* :539-549 */

/* ---- solver/cg_mms_tm.h:31: the single-flavour multi-shift CG (solver/cg_mms_tm.c:65-197) ----------------------------------
 * Device-resident (tmhip_cg_mms_tm) for M_psi = Qtm_pm_psi / Qsw_pm_psi with sdim = VOLUME/2 and M_psi = Q_pm_psi (no clover term)
 * with sdim = VOLUME, on unsplit lattices, up to 32 shifts.  Every other call (another M_psi, a T-split rank, more shifts) runs the
 * reference loop verbatim on host-visible fields in coherent mode, as cg_her's generic path does.  Either way
 * *cgmms_reached_prec receives the last err and g_sloppy_precision (when the host program has it) is reset to 0 (:175,192). */
int cg_mms_tm(spinor **const P, spinor *const Q, tmlqcd_solver_params *solver_params, double *cgmms_reached_prec);

/* ---- deriv_Sb.h: hopping part of the fermion force -------- */
typedef struct { double d1, d2, d3, d4, d5, d6, d7, d8; } su3adj;           /* su3adj.h:23-26 */
typedef struct {                                                             /* hamiltonian_field.h:26-32 */
  su3 **gaugefield;
  su3adj **momenta;
  su3adj **derivative;
  int update_gauge_copy;
  int traj_counter;
} hamiltonian_field_t;
/* deriv_Sb.c:401.  Coherent mode: the contribution is added to hf->derivative before returning.  Resident mode: it
 * stays in the device accumulator until tmlqcd_hip_flush_derivative(hf) adds it to hf->derivative (call that once,
 * after the last deriv_Sb of a force computation, e.g. at the end of det_derivative, monomial/det_monomial.c:56-117). */
void deriv_Sb(const int ieo, spinor *const l, spinor *const k, hamiltonian_field_t *const hf, const double factor);
void tmlqcd_hip_flush_derivative(hamiltonian_field_t *const hf);
/* the clover part of cloverdet_derivative (monomial/cloverdet_monomial.c:67-72,125-147) with swm / swp resident in HBM: replace the
 * zeroing loop, sw_spinor_eo (operator/clover_deriv.c:252), sw_deriv (:72) and sw_all (operator/clover_accumulate_deriv.c:58) calls;
 * the derivative follows the same coherent / resident rule as deriv_Sb */
void tmlqcd_hip_swpm_zero(void);
void tmlqcd_hip_sw_spinor_eo(const int ieo, const spinor *const kk, const spinor *const ll, const double fac);
void tmlqcd_hip_sw_deriv(const int ieo, const double mu);
void tmlqcd_hip_sw_all(hamiltonian_field_t *const hf, const double kappa, const double c_sw);

/* Molecular-dynamics link update with the links resident in HBM: replaces the call update_gauge(step, hf)
 * (update_gauge.c:51-110, called from the integrators, integrator.c) -- under its own name because the reference's
 * update_gauge.o stays on the link line for programs that do not want it.  Coherent mode: hf->gaugefield is current when
 * the call returns.  Resident mode: the host links stay behind until tmlqcd_hip_sync_gauge_to_host(hf) (call it before
 * host code reads g_gauge_field: gauge-action force, measurements, I/O).  tmlqcd_hip_update_momenta is update_momenta.c:67-72
 * for a derivative accumulated on the device only (resident deriv_Sb / tmlqcd_hip_sw_all). */
void tmlqcd_hip_update_gauge(const double step, hamiltonian_field_t *const hf);
void tmlqcd_hip_sync_gauge_to_host(hamiltonian_field_t *const hf);
void tmlqcd_hip_update_momenta(const double step, hamiltonian_field_t *const hf);
void tmlqcd_hip_sync_momenta_to_host(hamiltonian_field_t *const hf);

/* The frame of a trajectory with links and momenta resident in HBM: replace the host loops of update_tm.c around the integrator and the
 * norm loop of monitor_forces.c (INTEGRATION.md section 2.3c has the listing).  All under tmlqcd_hip_ names: moment_energy and
 * monitor_forces stay the reference's own symbols.  Residency rules as tmlqcd_hip_update_gauge / tmlqcd_hip_update_momenta:
 *   _gauge_snapshot       the loop update_tm.c:109-121.  The device links are brought up to date first (a raised g_update_gauge_copy is
 *                         honoured: the host's links go up), then copied into the device's gauge_tmp.  The host's gauge_tmp is not needed.
 *   _moment_energy        moment_energy(hf->momenta): uploads hf->momenta unless the momenta are resident (after tmlqcd_hip_update_momenta);
 *                         returns the sum over all ranks, the same bits on every rank.
 *   _gauge_snapshot_diff  update_tm.c:233-277: ret_gauge_diff between the device links and the snapshot, summed over all ranks.
 *   _accept_links         :313-328 (reunitarize = !bc_flag: restoresu3_in_place on every link; 0: the links stay) and :344-346.
 *   _reject_links         :329-339 (links <- snapshot) and :344-346.  The snapshot wins, as gauge_tmp does: a g_update_gauge_copy raised by
 *                         the host since tmlqcd_hip_gauge_snapshot is dropped, not answered with an upload.
 *                         After both, coherent and lazy mode: hf->gaugefield holds the device's links, the host's backward copy is refreshed,
 *                         g_update_gauge_copy and hf->update_gauge_copy are down, g_update_gauge_copy_32 is up, and the next operator
 *                         uploads nothing.  Resident mode: the host's links stay behind until tmlqcd_hip_sync_gauge_to_host.  In every
 *                         mode the clover blocks are stale (sw_term / sw_invert again, as after update_gauge), and the device's momenta are
 *                         given up without a download: the trajectory is over, the next tmlqcd_hip_update_momenta / _update_gauge /
 *                         _moment_energy uploads hf->momenta, which random_su3adj_field has drawn anew by then.
 *   _force_norms          monitor_forces.c:64-97: sum and maximum over the links of all ranks of _su3adj_square_norm of the DEVICE's derivative
 *                         accumulator.  Meant for a force accumulated on the device and not yet flushed (resident mode, between the
 *                         derivative functions and tmlqcd_hip_flush_derivative / tmlqcd_hip_update_momenta).  Otherwise it returns the norms
 *                         of what the accumulator still holds -- the force last flushed or consumed, never contributions other code added to
 *                         hf->derivative on the host -- and 0, 0 if no force has run on the device yet.
 * What stays on the host: random_su3adj_field (ranlxd is sequential and its numbers must be the reference's; enep stays the value it
 * returns) and the acceptance draw ranlxd(yy, 1). */
void tmlqcd_hip_gauge_snapshot(hamiltonian_field_t *const hf);
double tmlqcd_hip_moment_energy(hamiltonian_field_t *const hf);
double tmlqcd_hip_gauge_snapshot_diff(hamiltonian_field_t *const hf);
void tmlqcd_hip_accept_links(hamiltonian_field_t *const hf, const int reunitarize);
void tmlqcd_hip_reject_links(hamiltonian_field_t *const hf);
void tmlqcd_hip_force_norms(hamiltonian_field_t *const hf, double *sum, double *max);
/* whole-field copies across the bus so far: gauge uploads, gauge downloads, momenta uploads, momenta downloads (tmhip_transfer_counts) */
void tmlqcd_hip_transfer_counts(unsigned long out[4]);

/* ---- residency control (additions; not in the reference) ------------------- */
/* COHERENT (default): every call uploads its inputs and downloads its outputs -- exact drop-in, PCIe-bound.
 * RESIDENT: outputs stay in HBM until tmlqcd_hip_sync_to_host; the host program says when it touches a field.
 * LAZY: as RESIDENT, but the library finds out by itself: the pages of a host array whose current copy is in HBM are made
 *   inaccessible, the host's first load from one of them faults and fetches that page (or, if it keeps reading or stores, the field);
 *   arrays the device has read are write-protected, so a host store invalidates the mirror.  An UNMODIFIED host program then runs its
 *   stencil / operator loops at the HBM rate (also: environment TMLQCD_HIP_RESIDENCY=lazy).  Opt-in, for two reasons.  System calls
 *   do not fault: a field passed to write(2) / MPI while its host copy is stale must be synchronised first (tmlqcd_hip_sync_to_host).
 *   And arrays that go back to the allocator: a block the allocator unmaps (glibc: anything above its mmap threshold; the library
 *   leaves the program's malloc settings alone) is recognised when its address comes back -- a watched mirror is probed before it is
 *   trusted.  An array INSIDE a malloc arena (the main heap or a thread's: glibc serves a request from an arena whenever a free chunk
 *   fits), or in a shared / file-backed / named mapping, is never watched -- recognised from /proc/self/maps when it is first seen, it is
 *   copied on every call as in the coherent mode.  tmLQCD's fields, one calloc of hundreds of MB, are mappings of their own.  The SIGSEGV
 *   handler allocates nothing.  TMLQCD_HIP_LAZY_DEBUG=1 in the environment reports which arrays are not watched and why, and a SIGSEGV that
 *   is not the library's before it is passed on to the program's own handler. */
enum { TMLQCD_HIP_COHERENT = 0, TMLQCD_HIP_RESIDENT = 1, TMLQCD_HIP_LAZY = 2 };
/* Device versions of sw_term(g_gauge_field, kappa, c_sw) / sw_invert(ieo, mu) (operator/clover_term.c:88,
 * operator/clover_invert.c:170).  They carry their own names because the reference keeps other, unrelated functions in
 * the same objects (sw_invert_nd, six_invert ...), so those objects stay on the link line; replace the two calls
 * in operator.c:329-330,364 / the clover monomials to use them.  The host's sw / sw_inv arrays receive copies. */
void tmlqcd_hip_sw_term(const double kappa, const double c_sw);
void tmlqcd_hip_sw_invert(const int ieo, const double mu);
void tmlqcd_hip_set_residency(int mode);
/* lazy mode counters: page faults served, pages fetched one by one, whole-field fetches, host stores noticed */
void tmlqcd_hip_lazy_stats(unsigned long out[4]);
/* Upper bound on the number of device mirrors kept for host arrays (default 64, also TMLQCD_HIP_MAX_MIRRORS): beyond it the
 * least recently used mirror whose host copy is current is freed.  Host programs that allocate work fields per solve
 * (solver/solver_field.c) hand in ever new addresses; mirrors holding device-only data (resident mode) are never dropped. */
void tmlqcd_hip_set_max_mirrors(int n);
unsigned long tmlqcd_hip_calls(void);   /* number of reference-named entry points served so far (integration checks) */
void tmlqcd_hip_sync_to_host(spinor *field);       /* download the device mirror of `field` if it is newer */
void tmlqcd_hip_sync_all_to_host(void);
void tmlqcd_hip_host_modified(spinor *field);      /* the host wrote `field`: drop its device mirror */
void tmlqcd_hip_forget(spinor *field);             /* host memory is being freed: drop the mirror */
void tmlqcd_hip_set_device(int device);            /* before the first call; default: $TMLQCD_HIP_DEVICE or 0 */
void tmlqcd_hip_comm_init(const char unique_id[128]); /* ranks along T: id from tmhip_comm_get_unique_id, MPI_Bcast by the host */
void tmlqcd_hip_finalize(void);
/* ---- gauge monomial (monomial/gauge_monomial.c): replaces measure_gauge_action.o and measure_rectangles.o ------------------------
 * The three measures under the reference's names, on the device links: gf must be g_gauge_field (hf->gaugefield); it is uploaded by
 * the rule of every other entry point (g_update_gauge_copy), and in resident mode the device's newer links are measured without any
 * transfer.  measure_gauge_action also stores its result in GaugeInfo.plaquetteEnergy (measure_gauge_action.c:187).  On T-split ranks
 * the measures return the sum over all ranks (the reference's MPI_Allreduce); rectangles are not available there and end the program.
 * tmlqcd_hip_gauge_derivative is the body of gauge_derivative (glambda = 0) / gauge_EMderivative with the monomial's parameters as
 * arguments (beta = g_beta, c0 / c1 / use_rectangles / glambda of monomial_list[id]); it accumulates like tmlqcd_hip_sw_all. */
double measure_plaquette(const su3 **const gf);                                  /* measure_gauge_action.c:46 */
double measure_gauge_action(const su3 **const gf, const double lambda);          /* measure_gauge_action.c:108 */
double measure_rectangles(const su3 **const gf);                                 /* measure_rectangles.c:51 */
void tmlqcd_hip_gauge_derivative(hamiltonian_field_t *const hf, const double beta, const double c0, const double c1, const int use_rectangles, const double glambda);

/* ---- gradient flow (meas/gradient_flow.c, meas/measure_clover_field_strength_observables.c): replaces
 *      meas/measure_clover_field_strength_observables.o -----------------------------------------------------------------------------
 * measure_clover_field_strength_observables under the reference's name, on the device links: gf must be g_gauge_field, uploaded by the
 * rule of every other entry point; in resident mode the device's newer links are measured without any transfer.
 * tmlqcd_hip_gradient_flow_measurement is the body of gradient_flow_measurement with gf_eps / gf_tmax of measurement_list[id] as
 * arguments: it flows device copies of the links (neither g_gauge_field nor the resident links change) and writes gradflow.<traj>
 * (%06d) into the working directory in the reference's format.  An unopenable file and a T-split run end the program with a message. */
typedef struct { double E; double Q; } field_strength_obs_t;                     /* meas/field_strength_types.h */
void measure_clover_field_strength_observables(const su3 **const gf, field_strength_obs_t *const fso);
void tmlqcd_hip_gradient_flow_measurement(const int traj, const double eps, const double tmax);

/* ---- the other online measurements (meas/correlators.c, meas/pion_norm.c, meas/oriented_plaquettes.c, meas/polyakov_loop.c): replaces
 *      meas/oriented_plaquettes.o ---------------------------------------------------------------------------------------------------
 * tmlqcd_hip_slice_correlators: the sums of the t loop of correlators_measurement (dir 0: pp / pa / p4 hold T values each, what the
 * loop calls res / respa / resp4 before its MPI_Reduce) and of the z loop of pion_norm_measurement (dir 3: LZ values; pa = p4 = NULL),
 * taken from the two e/o halves of the propagator (optr->prop0 / prop1, g_spinor_field[2] / [3]) without convert_eo_to_lexic.  The
 * halves are registered like any other input: in lazy or resident mode nothing travels.  Any other dir ends the program.
 * measure_oriented_plaquettes and oriented_plaquettes_measurement under the reference's names, on the device links (gf must be
 * g_gauge_field, by the rules of measure_plaquette); the second appends its line to oriented_plaquettes.data in the working directory
 * and ends the program with a message when the file cannot be opened, as fatal_error does.
 * tmlqcd_hip_polyakov_loop: pl[0] + i pl[1] = the Polyakov loop along dir = 0 .. 3 (for 2 and 3 the value of polyakov_loop).
 * tmlqcd_hip_polyakov_loop_dir is polyakov_loop_dir: dir 0 or 3 (-1 otherwise), one line "nstore dir re im" written to
 * polyakovloop_dir<dir> (mode "w" for nstore == 0, "a" otherwise); 0 on success, -1 when the file cannot be opened.
 * The two gauge measurements end the program on T-split runs (g_nproc_t > 1). */
void tmlqcd_hip_slice_correlators(const spinor *const even, const spinor *const odd, const int dir, double *const pp, double *const pa, double *const p4);
void measure_oriented_plaquettes(const su3 **const gf, double *plaq);            /* meas/oriented_plaquettes.c:39 */
void oriented_plaquettes_measurement(const int traj, const int id, const int ieo); /* meas/oriented_plaquettes.c:88 */
void tmlqcd_hip_polyakov_loop(double pl[2], const int dir);
int tmlqcd_hip_polyakov_loop_dir(const int nstore, const int dir);               /* meas/polyakov_loop.c:325 */

/* ---- LapH: the 3D Laplacian on a time-slice and the eigensystem of all of them (jacobi.h, solver/eigenvalues_Jacobi.c) -------------
 * Jacobi under its reference name (the build with WITHLAPH, no MPI): l = Jacobi(k, t) on the device links; l and k are host vectors of
 * SPACEVOLUME su3_vector, copied in and out through two colour-vector fields of the session (they are NOT kept in the registry of
 * resident fields: every call moves its slice both ways).  l == k, a t outside [0, T) and a T-split run end the program.
 * tmlqcd_hip_laph_eigensystem stands in for the loop over the time-slices of eigenvalues_Jacobi.c: the nev lowest eigenpairs of every
 * slice by tmhip_laph_eigensystem (absolute prec on the residual, at most max_apps applications per slice), written into the working
 * directory as that file's branch without MPI writes them: eigenvalues.%.3d.%.4d (tslice, nstore) and eigenvector.%.3d.%.3d.%.4d (ev,
 * tslice, nstore).  Returns the number of slices on which all nev pairs converged.
 * Not built: Lemon / MPI output, jdher_su3vect and cg_her_su3vect, the smearing of the links before the Laplacian. */
void Jacobi(su3_vector *const l, su3_vector *const k, int t);
int tmlqcd_hip_laph_eigensystem(const int nev, const double prec, const int max_apps, const int nstore);

/* ---- rational monomials (monomial/ndrat_monomial.c type NDRAT, monomial/rat_monomial.c type RAT) --------------------------------------
 * The bodies of the three monomial functions with the monomial's parameters as arguments (rational_t::mu / rmu / nu / rnu with np entries,
 * EVMaxInv, maxiter, forceprec or accprec, g_relative_precision_flag), as tmlqcd_hip_gauge_derivative does for the gauge monomial; the
 * shifted solutions and work fields stay in HBM.  pf / pf2 are host pseudofermion fields, registered like any other field.  Unsplit
 * lattices only.  ndrat reads g_mubar, g_epsbar and phmc_invmaxev as the doublet operators do; rat runs at g_mu = 0 and leaves g_mu alone.
 *   *_derivative  ndrat_monomial.c:96-160 / rat_monomial.c:83-132: accumulates like deriv_Sb (added to hf->derivative before returning in
 *                 coherent mode, held on the device until tmlqcd_hip_flush_derivative / tmlqcd_hip_update_momenta in resident mode)
 *   *_heatbath    :212-254 / :175-199: pf (pf2) hold the Gaussian field on entry and the pseudofermion field on exit; *energy0 = |eta|^2
 *   *_acc         :281-309 / :232-250: *energy1; the caller forms energy1 - energy0
 * All return the solver's iteration count (what the reference adds to mnl->iter0 / iter1). */
int tmlqcd_hip_ndrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np,
                                const double EVMaxInv, const int max_iter, const double eps_sq, const int rel_prec);
int tmlqcd_hip_ndrat_heatbath(spinor *const pf, spinor *const pf2, const double *nu, const double *rnu, const int np, const double EVMaxInv,
                              const int max_iter, const double eps_sq, const int rel_prec, double *energy0);
int tmlqcd_hip_ndrat_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np, const int max_iter,
                         const double eps_sq, const int rel_prec, double *energy1);
/* ---- the polynomial monomial NDPOLY (monomial/ndpoly_monomial.c, Ptilde_nd.h, linalg/assign_mul_add_mul_add_mul_add_mul_r.h) ----
 * fp64, unsplit lattices, the branch g_epsbar != 0 || phmc_exact_poly == 0.  Not built: type NDCLOVER (cloverndpoly), the phmc_exact_poly == 1
 * branches, fp32 twins, T-split ranks (phmc_compute_ev of ndpoly_monomial.c:176: tmlqcd_hip_phmc_compute_ev, below).
 * assign_mul_add_mul_add_mul_add_mul_r: N = VOLUME/2 (or 0).  Ptilde_ndpsi: Qsq = &Qtm_pm_ndpsi or &Qsw_pm_ndpsi, any other ends the program
 * with a message; phmc_cheb_evmin / phmc_cheb_evmax are read at call time (weak references: a host program without them cannot call it).
 * The three bodies take what the reference's bodies read from the monomial; the caller keeps ndpoly_set_global_parameter (g_mubar, g_epsbar)
 * and, for the heatbath, draws the Gaussian field into pf / pf2 itself.  They end the program with a message when phmc_exact_poly == 1.
 *   _derivative  ndpoly_monomial.c:69-117, added to hf->derivative under the flush rules of tmlqcd_hip_ndrat_derivative; returns 0
 *   _heatbath    :179-209, 255-256: pf / pf2 = Ptilde B^dagger Q eta, *energy0 = |eta|^2; returns 0
 *   _acc         :282-368: *energy1 = mnl->energy1; returns the number of correction steps taken */
void assign_mul_add_mul_add_mul_add_mul_r(spinor *const R, spinor *const S, spinor *const U, spinor *const V, const double c1, const double c2,
                                          const double c3, const double c4, const int N);
void Ptilde_ndpsi(spinor *R_s, spinor *R_c, double *dd, int n, spinor *S_s, spinor *S_c, matrix_mult_nd Qsq);
int tmlqcd_hip_ndpoly_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots,
                                 const int MDPolyDegree, const double MDPolyLocNormConst, const double EVMaxInv);
int tmlqcd_hip_ndpoly_heatbath(spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots, const int MDPolyDegree,
                               const double MDPolyLocNormConst, const double EVMaxInv, const double *PtildeCoefs, const int PtildeDegree,
                               const double EVMin, double *energy0);
int tmlqcd_hip_ndpoly_acc(spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots, const int MDPolyDegree, const double MDPolyLocNormConst,
                          const double EVMaxInv, const double *MDPolyCoefs, const double *PtildeCoefs, const int PtildeDegree, const double EVMin,
                          const double PrecisionHfinal, double *energy1);
/* ---- the eigenvalue measurement (solver/eigenvalues_bi.h, phmc.c:205-253, solver/eigenvalues.c:162-229) ----
 * Thick-restart Lanczos on the device (tmhip_eigenvalues / tmhip_eigenvalues_nd of tmlqcd_hip.h) where the reference runs jdher /
 * jdher_bi on LAPACK with host vectors; the basis never leaves the device.  Unsplit lattices, fp64.  The residency rules are those of
 * the solvers; the doublet reads g_mubar, g_epsbar and phmc_invmaxev at the call.
 *   eigenvalues_bi     under its reference name.  Qsq is recognised BY ADDRESS as &Qtm_pm_ndbipsi or &Qsw_pm_ndbipsi -- the reference's
 *                      functions, declared weak here and never called (there are no bispinor data on the device) --, any other pointer
 *                      ends the program with a message.  maxmin 0 lowest, 1 highest (JD_MINIMAL / JD_MAXIMAL).  Returns the first
 *                      eigenvalue and sets *nev to the number converged (eigenvalues_bi.c:148-151); max_iterations bounds the restarts:
 *                      the run takes at most max_iterations Lanczos cycles (option "eig_restarts" of tmlqcd_hip.h around the call).
 *                      For &Qsw_pm_ndbipsi, and for clover != 0 below, the device's clover term must belong to the current links
 *                      (tmlqcd_hip_sw_term, or the host's sw_term followed by tmlqcd_hip_update_clover) and sw_invert_nd(mubar^2 -
 *                      epsbar^2) must have run on it, as for every symbol of the clover doublet above; otherwise the program ends
 *                      with the core's message.
 *   tmlqcd_hip_phmc_compute_ev   the body of phmc.c:205-253 for the monomial `name` with its EVMin: the lowest, then the highest
 *                      eigenvalue of Qtm_pm_ndpsi (clover = 0) or Qsw_pm_ndpsi (clover != 0) to `prec` (eigenvalue_precision), the two
 *                      warnings on stderr, and the line "%.8d %1.5e %1.5e %1.5e %1.5e\n" appended to monomial-<id>.data.  *ev_min, *ev_max
 *                      (may be NULL) receive the two values.  Returns 0.
 *   tmlqcd_hip_eigenvalues   the single-flavour case, in place of the jdher calls of eigenvalues.c:162-229: Qtm_pm_psi on VOLUME/2 sites
 *                      when even_odd_flag is set, Q_pm_psi on VOLUME sites otherwise.  evals[0 .. *nev) and, when evecs is not NULL, the
 *                      unit eigenvectors evecs[i * VOLUMEPLUSRAND/2 ...] (even_odd_flag) or evecs[i * VOLUMEPLUSRAND ...] in the host layout;
 *                      *nev = the number converged; returns evals[0].  The files and the globals eigenvectors / eigenvls / inv_eigenvls
 *                      stay the caller's.
 * Not built: interior eigenvalues and index_jd, the deflation globals, eigenvalues_Jacobi / jdher_su3vect, T-split ranks. */
typedef struct { spinor sp_up, sp_dn; } bispinor;                                      /* su3.h:70-73 */
typedef void (*matrix_mult_bi)(bispinor *const, bispinor *const);                     /* solver/matrix_mult_typedef.h:34 */
/* (Qtm_pm_ndbipsi and Qsw_pm_ndbipsi of operator/tm_operators_nd.h stay the host program's: the library refers to them weakly) */
double eigenvalues_bi(int *nev, const int max_iterations, const double prec, const int maxmin, matrix_mult_bi Qsq);
int tmlqcd_hip_phmc_compute_ev(const int trajectory_counter, const int id, const char *name, const double EVMin, const int clover,
                               const double prec, double *ev_min, double *ev_max);
double tmlqcd_hip_eigenvalues(int *nev, const int max_iterations, const double prec, const int maxmin, spinor *evecs, double *evals);
/* type NDCLOVERRAT: the same three bodies on the clover doublet (Qsw_pm_ndpsi, Qsw_tau1_sub_const_ndpsi, H_eo_sw_ndpsi).  The derivative also
 * does the clover part of ndrat_monomial.c:80-86, :162-184 on the device: swm / swp zeroed, four sw_spinor_eo per shift, sw_deriv_nd(EE)
 * when trlog is set, sw_all(kappa, c_sw).  The caller runs tmlqcd_hip_sw_term and sw_invert_nd(mubar^2 - epsbar^2) first (:89-91).  The
 * clover term must come from tmlqcd_hip_sw_term (it keeps the links sw_all walks): with the host's own sw_term + tmlqcd_hip_update_clover
 * the operators and solvers run, the derivative ends the program with a message before it touches anything. */
int tmlqcd_hip_ndcloverrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np,
                                      const double EVMaxInv, const double kappa, const double c_sw, const int trlog, const int max_iter,
                                      const double eps_sq, const int rel_prec);
int tmlqcd_hip_ndcloverrat_heatbath(spinor *const pf, spinor *const pf2, const double *nu, const double *rnu, const int np, const double EVMaxInv,
                                    const int max_iter, const double eps_sq, const int rel_prec, double *energy0);
int tmlqcd_hip_ndcloverrat_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np, const int max_iter,
                               const double eps_sq, const int rel_prec, double *energy1);
/* type CLOVERRAT of rat_monomial.c: the three bodies on Qsw_pm_psi / Qsw_plus_psi / H_eo_sw_inv_psi at g_mu = g_mu3 = 0 (both left alone).  The
 * derivative also does the clover part of rat_monomial.c:66-73, :113-116, :134-139 on the device: swm / swp zeroed, two sw_spinor_eo per shift
 * (summed per group of shifts in one launch per parity), sw_deriv(EE, 0.) when trlog is set, sw_all(kappa, c_sw).  The caller runs
 * tmlqcd_hip_sw_term and tmlqcd_hip_sw_invert(EE, 0.) first (:76-78); with an inverse made for another parity or mu, or a clover term that came
 * from the host (tmlqcd_hip_update_clover), the three calls end the program with a message before they touch anything. */
int tmlqcd_hip_cloverrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, const double *mu, const double *rmu, const int np, const double kappa,
                                    const double c_sw, const int trlog, const int max_iter, const double eps_sq, const int rel_prec);
int tmlqcd_hip_cloverrat_heatbath(spinor *const pf, const double *nu, const double *rnu, const int np, const int max_iter, const double eps_sq,
                                  const int rel_prec, double *energy0);
int tmlqcd_hip_cloverrat_acc(spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter, const double eps_sq,
                             const int rel_prec, double *energy1);
int tmlqcd_hip_rat_derivative(hamiltonian_field_t *const hf, spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter,
                              const double eps_sq, const int rel_prec);
int tmlqcd_hip_rat_heatbath(spinor *const pf, const double *nu, const double *rnu, const int np, const int max_iter, const double eps_sq,
                            const int rel_prec, double *energy0);
int tmlqcd_hip_rat_acc(spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter, const double eps_sq,
                       const int rel_prec, double *energy1);
/* ---- correction monomials (monomial/ratcor_monomial.c types RATCOR / CLOVERRATCOR, monomial/ndratcor_monomial.c types NDRATCOR /
 * NDCLOVERRATCOR): the series loops of the heatbath (ratcor_monomial.c:85-110, ndratcor_monomial.c:88-123) and of the acceptance step
 * (:151-168, :166-187) with apply_Z_psi / apply_Z_ndpsi inside, everything but pf (pf2) in HBM.  mu / rmu / A: rational_t::mu, rmu, A with np
 * entries; accprec is the solver's squared precision and the stopping threshold of the series (mnl->accprec); max_iter = mnl->maxiter,
 * rel_prec = g_relative_precision_flag.  The caller draws the Gaussian field into pf (pf2) before the heatbath, which returns *energy0 =
 * |eta|^2; the acceptance step returns *energy1.  *napp (may be NULL): applications of Z.  Return value: what the call adds to mnl->iter0.
 * The single-flavour bodies run at g_mu = g_mu3 = 0, the doublet bodies at g_mu3 = 0 and with g_mubar, g_epsbar as the doublet operators read
 * them; the globals are left alone.  Clover types: the caller runs tmlqcd_hip_sw_term and tmlqcd_hip_sw_invert(EE, 0.), respectively
 * sw_invert_nd(mubar^2 - epsbar^2), first, as the reference's bodies do; otherwise the call ends the program with a message.
 * The reference's loops can apply Z a seventh time and then read past coefs[6]; these bodies end the program with a message naming delta and
 * accprec when the sixth application leaves delta >= accprec.  Unsplit lattices only.  Not built: check_C_psi / check_C_ndpsi (phmc_compute_ev: tmlqcd_hip_phmc_compute_ev). */
int tmlqcd_hip_ratcor_heatbath(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                               const double accprec, const int rel_prec, double *energy0, int *napp);
int tmlqcd_hip_ratcor_acc(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter, const double accprec,
                          const int rel_prec, double *energy1, int *napp);
int tmlqcd_hip_cloverratcor_heatbath(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                                     const double accprec, const int rel_prec, double *energy0, int *napp);
int tmlqcd_hip_cloverratcor_acc(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                                const double accprec, const int rel_prec, double *energy1, int *napp);
int tmlqcd_hip_ndratcor_heatbath(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                 const int max_iter, const double accprec, const int rel_prec, double *energy0, int *napp);
int tmlqcd_hip_ndratcor_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                            const double accprec, const int rel_prec, double *energy1, int *napp);
int tmlqcd_hip_ndcloverratcor_heatbath(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                       const int max_iter, const double accprec, const int rel_prec, double *energy0, int *napp);
int tmlqcd_hip_ndcloverratcor_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                  const int max_iter, const double accprec, const int rel_prec, double *energy1, int *napp);

/* ---- ILDG gauge configurations: replaces io/gauge_read.o and io/gauge_write.o of libio.a -- */
typedef struct { unsigned int suma, sumb; } DML_Checksum;                        /* io/dml.h:34-37 */
typedef struct {                                                                 /* io/params.h:98-104 */
  double plaquetteEnergy;
  int gaugeRead;
  DML_Checksum checksum;
  char *xlfInfo;
  char *ildg_data_lfn;
} paramsGaugeInfo;
typedef struct {                                                                 /* io/params.h:71-88 */
  char date[64];
  char package_version[32];
  double beta, c2_rec, epsilonbar, kappa, mu, mubar, plaq;
  int counter;
  long int time;
} paramsXlfInfo;
extern paramsGaugeInfo GaugeInfo;                                                /* io/gauge_read.c:27 */
/* reads gauge_precision_read_flag and g_disable_IO_checks at call time (both optional: weak references, defaults 64 / checks on) */
int read_gauge_field(char *filename, su3 **const gf);                            /* io/gauge.h, io/gauge_read.c:28 */
int write_gauge_field(char *filename, const int prec, paramsXlfInfo const *xlfInfo);   /* io/gauge_write.c:22 */
/* ---- propagators and sources: read_spinor replaces the function of that name in io/spinor_read.o, which stays in libio.a with the
 *      symbol localized (the object also defines PropInfo and SourceInfo) -- */
/* io/spinor.h, io/spinor_read.c:27: return values, messages and prints of the reference; r == NULL: s is a lexicographic field.  Reads
 * g_disable_src_IO_checks, g_debug_level and g_cart_id at call time (all optional: weak references, defaults 0, 1, 0).  The fields
 * follow the residency mode like any other output. */
int read_spinor(spinor *const s, spinor *const r, char *filename, const int position);
/* write_spinor(writer, s, r, flavours, prec) of io/spinor_write.c:23 on a file name instead of a c-lime WRITER: per flavour the
 * "scidac-binary-data" header, the record packed on the device and the "scidac-checksum" message are appended to (append != 0) or
 * start (append == 0) the file; r == NULL: lexicographic fields; at most 8 flavours.  tmlqcd_hip_write_lime_message writes one of
 * the message records around them with the caller's text.  Both return 0 or -1. */
int tmlqcd_hip_write_spinor(char *filename, const int append, spinor **const s, spinor **const r, const int flavours, const int prec);
int tmlqcd_hip_write_lime_message(char *filename, const int append, const char *type, const char *text, const int mb, const int me);
/* source_spinor_field (start.c:707) and source_spinor_field_point_from_file (start.c:743) on the device mirrors of P and Q; not under
 * their reference names: start.o holds the random number generator and stays on the link line */
void tmlqcd_hip_source_spinor_field(spinor *const P, spinor *const Q, int is, int ic);
void tmlqcd_hip_source_spinor_field_point_from_file(spinor *const P, spinor *const Q, int is, int ic, int source_indx);
/* benchmark.c:291-300 on device-resident mirrors; returns seconds for `iters` x {H(0,f1,f0); H(1,f2,f1)} */
double tmlqcd_hip_benchmark_loop(spinor *f0, spinor *f1, spinor *f2, int iters);

#ifdef __cplusplus
}
#endif
#endif
