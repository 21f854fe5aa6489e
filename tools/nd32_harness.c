/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_nd32.py together with the reference's own
 * operator/tm_operators_nd.c, operator/tm_operators_nd_32.c, solver/rg_mixed_cg_her_nd.c, solver/cg_her_nd.c and linalg/mul_r_32.c
 * (compiled in place into a temporary directory, with -D_USE_HALFSPINOR=1) and oracle/_ref/libtmref_hs.so, the half-spinor build,
 * which provides Hopping_Matrix, Hopping_Matrix_32, the linalg sets of both precisions, the solver fields, the geometry and the
 * globals (g_mubar, g_epsbar, g_spinor_field, g_spinor_field32, ...).
 *
 * What those five files need and libtmref_hs.so does not define: phmc_invmaxev (phmc.h:31), the symbols of the polynomial helpers
 * (P_ndpsi, Qtau1_P_ndpsi, ...) and the three callees of Qsw_pm_ndpsi_32, none of which the fixtures ever call -- defined here as
 * inert dummies. */
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
void tmnd32_set(double mubar, double epsbar, double invmaxev) { g_mubar = mubar; g_epsbar = epsbar; phmc_invmaxev = invmaxev; }

/* solver_params_t (solver/solver_params.h:70-100) is filled here so that the Python side need not mirror its layout */
#include "su3.h"
#include "solver/solver_params.h"
#include "solver/matrix_mult_typedef_nd.h"
extern int rg_mixed_cg_her_nd(spinor *const P_up, spinor *const P_dn, spinor *const Q_up, spinor *const Q_dn, solver_params_t solver_params,
                              const int max_iter, const double eps_sq, const int rel_prec, const int N, matrix_mult_nd f, matrix_mult_nd32 f32);
extern void Qtm_pm_ndpsi(spinor *const, spinor *const, spinor *const, spinor *const);
extern void Qtm_pm_ndpsi_32(spinor32 *const, spinor32 *const, spinor32 *const, spinor32 *const);
int tmnd32_rg_mixed_cg_her_nd(spinor *P_up, spinor *P_dn, spinor *Q_up, spinor *Q_dn, double delta, int max_iter, double eps_sq, int rel_prec,
                              int N) {
  solver_params_t sp;
  __builtin_memset(&sp, 0, sizeof(sp));
  sp.mcg_delta = (float)delta;
  return rg_mixed_cg_her_nd(P_up, P_dn, Q_up, Q_dn, sp, max_iter, eps_sq, rel_prec, N, &Qtm_pm_ndpsi, &Qtm_pm_ndpsi_32);
}

/* the doublet operators use g_spinor_field[DUM_MATRIX .. DUM_MATRIX+5]; oracle/ref_harness.c reserves three fields there */
extern int DUM_MATRIX, g_debug_level;
void tmnd32_set_dum(int dum) { DUM_MATRIX = dum; }
void tmnd32_set_debug(int level) { g_debug_level = level; }
