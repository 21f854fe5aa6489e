/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_mixed_mms.py together with the reference's own
 * solver/mixed_cg_mms_tm_nd.c, solver/cg_mms_tm_nd.c, operator/tm_operators_nd.c, operator/tm_operators_nd_32.c,
 * linalg/assign_mul_add_mul_r.c, linalg/assign_mul_add_mul_r_32.c and linalg/mul_r_32.c (compiled in place into a temporary
 * directory, with -D_USE_HALFSPINOR=1) and oracle/_ref/libtmref_hs.so, the half-spinor build, which provides Hopping_Matrix,
 * Hopping_Matrix_32, the linalg sets of both precisions, the solver fields, the geometry and the globals.
 *
 * What those files need and libtmref_hs.so does not define -- phmc_invmaxev (phmc.h:31), the symbols of the polynomial helpers and the
 * three callees of Qsw_pm_ndpsi_32, none of which the fixtures ever call -- is defined here as inert dummies, as in tools/nd32_harness.c. */
#include <complex.h>
#include <stddef.h>

double phmc_invmaxev = 1.0;
double phmc_Cpol = 1.0;
_Complex double *phmc_root = NULL;
int phmc_dop_n_cheby = 0;
void compact(void *R, void *S, void *P) { (void)R; (void)S; (void)P; }
void decompact(void *S, void *P, void *R) { (void)S; (void)P; (void)R; }
void assign_mul_one_sw_pm_imu_eps_32_orphaned(int ieo, void *k_s, void *k_c, void *l_s, void *l_c, float mu, float eps) {
  (void)ieo; (void)k_s; (void)k_c; (void)l_s; (void)l_c; (void)mu; (void)eps;
}
void clover_gamma5_nd_32_orphaned(int ieo, void *l_c, void *l_s, void *k_c, void *k_s, void *j_c, void *j_s, float mubar, float epsbar) {
  (void)ieo; (void)l_c; (void)l_s; (void)k_c; (void)k_s; (void)j_c; (void)j_s; (void)mubar; (void)epsbar;
}
void clover_inv_nd_32_orphaned(int ieo, void *l_c, void *l_s) { (void)ieo; (void)l_c; (void)l_s; }

extern double g_mubar, g_epsbar;
void tmmm_set(double mubar, double epsbar, double invmaxev) { g_mubar = mubar; g_epsbar = epsbar; phmc_invmaxev = invmaxev; }

/* solver_params_t (solver/solver_params.h:70-100) is filled here so that the Python side need not mirror its layout */
#include "su3.h"
#include "solver/solver_params.h"
extern int cg_mms_tm_nd(spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, solver_params_t *sp);
extern int mixed_cg_mms_tm_nd(spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, solver_params_t *sp);
extern void Qtm_pm_ndpsi(spinor *const, spinor *const, spinor *const, spinor *const);
extern void Qtm_pm_ndpsi_32(spinor32 *const, spinor32 *const, spinor32 *const, spinor32 *const);

/* mixed != 0: mixed_cg_mms_tm_nd, else cg_mms_tm_nd */
int tmmm_solve(int mixed, spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, double *shifts, int nshifts, int max_iter, double eps_sq,
               int rel_prec, int N) {
  solver_params_t sp;
  __builtin_memset(&sp, 0, sizeof(sp));
  sp.max_iter = max_iter; sp.rel_prec = rel_prec; sp.no_shifts = nshifts; sp.sdim = N;
  sp.squared_solver_prec = eps_sq; sp.shifts = shifts;
  sp.M_ndpsi = &Qtm_pm_ndpsi;
  sp.M_ndpsi32 = &Qtm_pm_ndpsi_32;
  return mixed ? mixed_cg_mms_tm_nd(Pup, Pdn, Qup, Qdn, &sp) : cg_mms_tm_nd(Pup, Pdn, Qup, Qdn, &sp);
}

/* the doublet operators use g_spinor_field[DUM_MATRIX .. DUM_MATRIX+5]; oracle/ref_harness.c reserves three fields there */
extern int DUM_MATRIX, g_debug_level;
void tmmm_set_dum(int dum) { DUM_MATRIX = dum; }
void tmmm_set_debug(int level) { g_debug_level = level; }
