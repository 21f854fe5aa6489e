/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_ndsw.py together with the reference's own operator/tm_operators_nd.c,
 * solver/cg_her_nd.c, solver/cg_mms_tm_nd.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c (compiled in place into a
 * temporary directory) and oracle/_ref/libtmref.so, which provides Hopping_Matrix, the clover functions (clover_term.c,
 * clover_invert.c, clovertm_operators.c, clover_deriv.c, clover_accumulate_deriv.c), deriv_Sb, the linalg set, the geometry and
 * the globals.
 *
 * What those files need and libtmref.so does not define: the phmc globals (phmc.h:29-35) and the helpers of the polynomial code
 * paths that the fixtures never call -- inert dummies, as in tools/nd_harness.c. */
#include <complex.h>
#include <stddef.h>

double phmc_invmaxev = 1.0;
double phmc_Cpol = 1.0;
_Complex double *phmc_root = NULL;
int phmc_dop_n_cheby = 0;
void compact(void *R, void *S, void *P) { (void)R; (void)S; (void)P; }
void decompact(void *S, void *P, void *R) { (void)S; (void)P; (void)R; }

extern double g_mubar, g_epsbar;
void tmndsw_set(double mubar, double epsbar, double invmaxev) { g_mubar = mubar; g_epsbar = epsbar; phmc_invmaxev = invmaxev; }

/* solver_params_t (solver/solver_params.h:70-100) is filled here so that the Python side need not mirror its layout */
#include "su3.h"
#include "solver/solver_params.h"
extern int cg_mms_tm_nd(spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, solver_params_t *sp);
extern void Qsw_pm_ndpsi(spinor *const, spinor *const, spinor *const, spinor *const);
int tmndsw_cg_mms_tm_nd(spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, double *shifts, int nshifts, int max_iter,
                        double eps_sq, int rel_prec, int N) {
  solver_params_t sp;
  __builtin_memset(&sp, 0, sizeof(sp));
  sp.max_iter = max_iter; sp.rel_prec = rel_prec; sp.no_shifts = nshifts; sp.sdim = N;
  sp.squared_solver_prec = eps_sq; sp.shifts = shifts;
  sp.M_ndpsi = &Qsw_pm_ndpsi;
  return cg_mms_tm_nd(Pup, Pdn, Qup, Qdn, &sp);
}

/* Qsw_pm_ndpsi uses g_spinor_field[DUM_MATRIX .. DUM_MATRIX+7]; oracle/ref_harness.c reserves three fields there */
extern int DUM_MATRIX, g_debug_level;
void tmndsw_set_dum(int dum) { DUM_MATRIX = dum; }
void tmndsw_set_debug(int level) { g_debug_level = level; }
