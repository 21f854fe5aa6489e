/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_mms.py together with the reference's own solver/cg_mms_tm.c and
 * linalg/assign_mul_add_mul_r.c (compiled in place into a temporary directory) and oracle/_ref/libtmref.so, which provides
 * Qtm_pm_psi, Qsw_pm_psi, Q_pm_psi, the linalg set, init_solver_field, the geometry and the globals (g_mu, g_sloppy_precision, ...).
 *
 * solver_params_t (solver/solver_params.h:46-109) is filled here so that the Python side need not mirror its layout. */
#include "su3.h"
#include "solver/solver_params.h"
extern int cg_mms_tm(spinor **const P, spinor *const Q, solver_params_t *solver_params, double *cgmms_reached_prec);
extern void Qtm_pm_psi(spinor *const, spinor *const);
extern void Qsw_pm_psi(spinor *const, spinor *const);
extern void Q_pm_psi(spinor *const, spinor *const);
extern int g_debug_level, g_sloppy_precision;

/* op 0: Qtm_pm_psi, 1: Qsw_pm_psi (both on N = VOLUME/2), 2: Q_pm_psi (N = VOLUME) */
int tmmms_cg_mms_tm(spinor **P, spinor *Q, double *shifts, int nshifts, int max_iter, double eps_sq, int rel_prec, int N, int op,
                    double *reached) {
  solver_params_t sp;
  __builtin_memset(&sp, 0, sizeof(sp));
  sp.max_iter = max_iter; sp.rel_prec = rel_prec; sp.no_shifts = nshifts; sp.sdim = N;
  sp.squared_solver_prec = eps_sq; sp.shifts = shifts;
  sp.M_psi = op == 0 ? &Qtm_pm_psi : (op == 1 ? &Qsw_pm_psi : &Q_pm_psi);
  return cg_mms_tm(P, Q, &sp, reached);
}
void tmmms_set_debug(int level) { g_debug_level = level; }
void tmmms_set_sloppy(int v) { g_sloppy_precision = v; }
int tmmms_get_sloppy(void) { return g_sloppy_precision; }
