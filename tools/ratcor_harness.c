/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_ratcor.py together with the reference's own solver/cg_mms_tm.c,
 * solver/cg_mms_tm_nd.c, operator/tm_operators_nd.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c (compiled in place
 * into a temporary directory) and oracle/_ref/libtmref.so, which provides Qtm_pm_psi, Qsw_pm_psi, the clover functions, the linalg
 * set, init_solver_field, the geometry and the globals.
 *
 * The correction monomials read everything from monomial_list[id], which this build does not have: the functions below call the
 * reference's own solvers, operators and linalg in the order of apply_Z_psi / apply_Z_ndpsi and of the four series loops
 * (monomial/ratcor_monomial.c, monomial/ndratcor_monomial.c), with the monomial's fields and numbers as arguments.  The loops stop
 * after six applications of Z (the length of the reference's coefficient tables) and say so in *napp = -6. */
#include <complex.h>
#include <stddef.h>
#include "su3.h"
#include "solver/solver_params.h"

/* what operator/tm_operators_nd.c needs and libtmref.so does not define: inert, as in tools/ndsw_harness.c */
double phmc_invmaxev = 1.0;
double phmc_Cpol = 1.0;
_Complex double *phmc_root = NULL;
int phmc_dop_n_cheby = 0;
void compact(void *R, void *S, void *P) { (void)R; (void)S; (void)P; }
void decompact(void *S, void *P, void *R) { (void)S; (void)P; (void)R; }

extern double g_mubar, g_epsbar, g_mu, g_mu3;
extern int DUM_MATRIX, g_debug_level;
extern int cg_mms_tm(spinor **const P, spinor *const Q, solver_params_t *solver_params, double *cgmms_reached_prec);
extern int cg_mms_tm_nd(spinor **Pup, spinor **Pdn, spinor *Qup, spinor *Qdn, solver_params_t *sp);
extern void Qtm_pm_psi(spinor *const, spinor *const);
extern void Qsw_pm_psi(spinor *const, spinor *const);
extern void Qtm_pm_ndpsi(spinor *const, spinor *const, spinor *const, spinor *const);
extern void Qsw_pm_ndpsi(spinor *const, spinor *const, spinor *const, spinor *const);
extern void assign(spinor *const R, spinor *const S, const int N);
extern void assign_add_mul_r(spinor *const P, spinor *const Q, const double c, const int N);
extern void mul_r(spinor *const R, const double c, spinor *const S, const int N);
extern void diff(spinor *const Q, spinor *const R, spinor *const S, const int N);
extern double square_norm(spinor *const P, const int N, const int parallel);
extern double scalar_prod_r(spinor *const S, spinor *const R, const int N, const int parallel);

void tmrc_set_nd(double mubar, double epsbar, double invmaxev) { g_mubar = mubar; g_epsbar = epsbar; phmc_invmaxev = invmaxev; }
void tmrc_set_mu(double mu, double mu3) { g_mu = mu; g_mu3 = mu3; }
void tmrc_set_dum(int dum) { DUM_MATRIX = dum; }
void tmrc_set_debug(int level) { g_debug_level = level; }

/* the monomial: nd 0 / 1 = ratcor / ndratcor, sw 0 / 1 = Qtm / Qsw; chi_*[np] is the field the reference multiplies into (:205) */
static struct {
  int nd, sw, np, N, iter0;
  spinor **chi_up, **chi_dn;
  double *mu, *rmu, A;
  solver_params_t sp;
} m;

void tmrc_monomial(int nd, int sw, spinor **chi_up, spinor **chi_dn, double *mu, double *rmu, double A, int np, int max_iter, double accprec,
                   int rel_prec, int N) {
  m.nd = nd; m.sw = sw; m.chi_up = chi_up; m.chi_dn = chi_dn; m.mu = mu; m.rmu = rmu; m.A = A; m.np = np; m.N = N; m.iter0 = 0;
  __builtin_memset(&m.sp, 0, sizeof(m.sp));
  m.sp.max_iter = max_iter; m.sp.squared_solver_prec = accprec; m.sp.no_shifts = np; m.sp.shifts = mu; m.sp.sdim = N; m.sp.rel_prec = rel_prec;
  m.sp.M_psi = sw ? &Qsw_pm_psi : &Qtm_pm_psi;
  m.sp.M_ndpsi = sw ? &Qsw_pm_ndpsi : &Qtm_pm_ndpsi;
}
int tmrc_iter0(void) { return m.iter0; }

static int solve(spinor *up, spinor *dn) {
  double reached;
  return m.nd ? cg_mms_tm_nd(m.chi_up, m.chi_dn, up, dn, &m.sp) : cg_mms_tm(m.chi_up, up, &m.sp, &reached);
}

/* ratcor_monomial.c:183-218, ndratcor_monomial.c:202-245 */
double tmrc_apply_Z(spinor *k_up, spinor *k_dn, spinor *l_up, spinor *l_dn) {
  const int N = m.N, np = m.np;
  m.iter0 += solve(l_up, l_dn);
  assign(k_up, l_up, N);
  if (m.nd) assign(k_dn, l_dn, N);
  for (int j = np - 1; j > -1; j--) {
    assign_add_mul_r(k_up, m.chi_up[j], m.rmu[j], N);
    if (m.nd) assign_add_mul_r(k_dn, m.chi_dn[j], m.rmu[j], N);
  }
  solve(k_up, k_dn);
  for (int j = np - 1; j > -1; j--) {
    assign_add_mul_r(k_up, m.chi_up[j], m.rmu[j], N);
    if (m.nd) assign_add_mul_r(k_dn, m.chi_dn[j], m.rmu[j], N);
  }
  mul_r(m.chi_up[np], m.A * m.A, k_up, N);
  if (m.nd) mul_r(m.chi_dn[np], m.A * m.A, k_dn, N);
  if (m.nd) m.sp.M_ndpsi(k_up, k_dn, m.chi_up[np], m.chi_dn[np]);
  else m.sp.M_psi(k_up, m.chi_up[np]);
  diff(k_up, k_up, l_up, N);
  if (m.nd) diff(k_dn, k_dn, l_dn, N);
  double resi = square_norm(k_up, N, 1);
  if (m.nd) resi += square_norm(k_dn, N, 1);
  return resi;
}

/* ratcor_monomial.c:87-110, ndratcor_monomial.c:90-123 after the random numbers; w[0..3] = w_fields[0..3]; deltas[6] */
double tmrc_heatbath(spinor *pf, spinor *pf2, spinor **w, double accprec, double *deltas, int *napp) {
  const double coefs[6] = {1. / 4., -3. / 32., 7. / 128., -77. / 2048., 231. / 8192., -1463. / 65536.};
  const int N = m.N;
  double energy0 = square_norm(pf, N, 1);
  if (m.nd) energy0 += square_norm(pf2, N, 1);
  m.iter0 = 0;
  assign(w[0], pf, N);
  if (m.nd) assign(w[1], pf2, N);
  spinor *up0 = w[0], *dn0 = w[1], *up1 = w[2], *dn1 = w[3], *tup, *tdn;
  *napp = -6;
  for (int i = 1; i < 7; i++) {
    const double delta = tmrc_apply_Z(up1, dn1, up0, dn0);
    deltas[i - 1] = delta;
    assign_add_mul_r(pf, up1, coefs[i - 1], N);
    if (m.nd) assign_add_mul_r(pf2, dn1, coefs[i - 1], N);
    if (delta < accprec) { *napp = i; break; }
    tup = up0; tdn = dn0;
    up0 = up1; dn0 = dn1;
    up1 = tup; dn1 = tdn;
  }
  return energy0;
}

/* ratcor_monomial.c:151-168, ndratcor_monomial.c:166-187; w[0..5] = w_fields[0..5] */
double tmrc_acc(spinor *pf, spinor *pf2, spinor **w, double accprec, double *deltas, int *napp) {
  const double coefs[6] = {-1. / 2., 3. / 8., -5. / 16., 35. / 128., -63. / 256., 231. / 1024.};
  const int N = m.N;
  assign(w[4], pf, N);
  if (m.nd) assign(w[5], pf2, N);
  spinor *up0 = w[0], *dn0 = w[1], *up1 = w[2], *dn1 = w[3], *tup, *tdn;
  double delta = tmrc_apply_Z(up0, dn0, pf, pf2);
  deltas[0] = delta;
  assign_add_mul_r(w[4], up0, coefs[0], N);
  if (m.nd) assign_add_mul_r(w[5], dn0, coefs[0], N);
  int n = 1;
  for (int i = 2; i < 7; i++) {
    if (delta < accprec) break;
    delta = tmrc_apply_Z(up1, dn1, up0, dn0);
    deltas[i - 1] = delta;
    n = i;
    assign_add_mul_r(w[4], up1, coefs[i - 1], N);
    if (m.nd) assign_add_mul_r(w[5], dn1, coefs[i - 1], N);
    tup = up0; tdn = dn0;
    up0 = up1; dn0 = dn1;
    up1 = tup; dn1 = tdn;
  }
  *napp = delta < accprec ? n : -6;
  double energy1 = scalar_prod_r(pf, w[4], N, 1);
  if (m.nd) energy1 += scalar_prod_r(pf2, w[5], N, 1);
  return energy1;
}
