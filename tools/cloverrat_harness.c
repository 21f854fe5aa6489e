/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_cloverrat.py together with the reference's own operator/clover_det.c,
 * solver/cg_mms_tm.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c (compiled in place into a temporary directory) and
 * oracle/_ref/libtmref.so, which provides Qsw_pm_psi, Qsw_plus_psi, H_eo_sw_inv_psi, the clover functions (clover_term.c,
 * clover_invert.c, clover_deriv.c, clover_accumulate_deriv.c), deriv_Sb, the linalg set, init_solver_field, the geometry and the
 * globals.
 *
 * solver_params_t (solver/solver_params.h:46-109) is filled here so that the Python side need not mirror its layout. */
#include "su3.h"
#include "solver/solver_params.h"
extern int cg_mms_tm(spinor **const P, spinor *const Q, solver_params_t *solver_params, double *cgmms_reached_prec);
extern void Qsw_pm_psi(spinor *const, spinor *const);
extern int g_debug_level;

/* rat_monomial.c:83-93 for CLOVERRAT: M_psi = mnl->Qsq = Qsw_pm_psi on N = VOLUME/2 */
int tmcr_cg_mms_tm(spinor **P, spinor *Q, double *shifts, int nshifts, int max_iter, double eps_sq, int rel_prec, int N, double *reached) {
  solver_params_t sp;
  __builtin_memset(&sp, 0, sizeof(sp));
  sp.max_iter = max_iter; sp.rel_prec = rel_prec; sp.no_shifts = nshifts; sp.sdim = N;
  sp.squared_solver_prec = eps_sq; sp.shifts = shifts;
  sp.M_psi = &Qsw_pm_psi;
  return cg_mms_tm(P, Q, &sp, reached);
}
void tmcr_set_debug(int level) { g_debug_level = level; }
