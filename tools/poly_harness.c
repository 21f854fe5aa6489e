/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_poly.py together with the reference's own monomial/ndpoly_monomial.c, Ptilde_nd.c,
 * chebyshev_polynomial_nd.c, linalg/assign_mul_add_mul_add_mul_add_mul_r.c, operator/tm_operators_nd.c and init/init_chi_spinor_field.c
 * (compiled in place into a temporary directory) and oracle/_ref/libtmref.so, which provides Hopping_Matrix, the single-flavour
 * operators, the linalg set, deriv_Sb, the random numbers, the geometry and the globals.
 *
 * This file holds no algorithm: it defines the phmc globals (phmc.h) and the monomial list that the reference's files expect from
 * phmc.c and monomial/monomial.c, fills ONE monomial of type NDPOLY from the numbers of an input file, and calls the reference's
 * init_ndpoly_monomial / ndpoly_derivative / ndpoly_heatbath / ndpoly_acc.  What the other branches of those three bodies call
 * (phmc_exact_poly == 1, type NDCLOVER, the eigenvalue measurement) is never reached and ends the program if it is. */
#include <complex.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "global.h"
#include "su3.h"
#include "su3adj.h"
#include "start.h"
#include "hamiltonian_field.h"
#include "monomial/monomial.h"
#include "phmc.h"

double phmc_Cpol = 1.0, phmc_cheb_evmin = 0.0, phmc_cheb_evmax = 1.0, phmc_invmaxev = 1.0;
_Complex double *phmc_root = NULL;
int phmc_dop_n_cheby = 0, phmc_ptilde_n_cheby = 0, phmc_max_ptilde_degree = NTILDE_CHEBYMAX;
double *phmc_dop_cheby_coef = NULL, *phmc_ptilde_cheby_coef = NULL;
int phmc_exact_poly = 0;
monomial monomial_list[max_no_monomials];

void compact(void *R, void *S, void *P) { (void)R; (void)S; (void)P; }
void decompact(void *S, void *P, void *R) { (void)S; (void)P; (void)R; }

/* the eigenvalue measurement of the heatbath (ndpoly_monomial.c:175-177; rec_ev = 0 here) */
void phmc_compute_ev(const int trajectory_counter, const int id, matrix_mult_bi Qsq) {
  (void)trajectory_counter; (void)id; (void)Qsq;
  fprintf(stderr, "poly_harness: phmc_compute_ev reached\n");
  exit(7);
}

/* the solver of the phmc_exact_poly == 1 heatbath (ndpoly_monomial.c:220) */
int cg_her_nd(void) {
  fprintf(stderr, "poly_harness: cg_her_nd reached\n");
  exit(7);
}

extern int DUM_MATRIX;
void tmpoly_set_dum(int dum) { DUM_MATRIX = dum; }

static su3adj *df = NULL, **dfp = NULL;
static hamiltonian_field_t hf;
double *tmpoly_derivative(void) {
  if (!df) {
    df = calloc((size_t)4 * VOLUMEPLUSRAND, sizeof(su3adj));
    dfp = malloc((size_t)VOLUMEPLUSRAND * sizeof(su3adj *));
    for (int i = 0; i < VOLUMEPLUSRAND; i++) dfp[i] = df + 4 * (size_t)i;
  }
  hf.gaugefield = g_gauge_field; hf.momenta = NULL; hf.derivative = dfp; hf.update_gauge_copy = 0; hf.traj_counter = 1;
  return (double *)df;
}

/* the numbers of the monomial's input block (read_input.l) and the fields it owns; then the reference's own initialisation */
int tmpoly_init(double kappa, double mubar, double epsbar, double stilde_min, double stilde_max, double locnorm, double precision_ptilde,
                int degree, double precision_hfinal, const char *roots_file, spinor *pf, spinor *pf2, spinor *w0, spinor *w1, int debug) {
  monomial *mnl = &monomial_list[0];
  static spinor *w[2];
  memset(mnl, 0, sizeof(*mnl));
  mnl->type = NDPOLY;
  strcpy(mnl->name, "ndpoly");
  mnl->kappa = kappa; mnl->mubar = mubar; mnl->epsbar = epsbar; mnl->c_sw = 0.0;
  mnl->StildeMin = stilde_min; mnl->StildeMax = stilde_max; mnl->MDPolyLocNormConst = locnorm;
  mnl->PrecisionPtilde = precision_ptilde; mnl->MDPolyDegree = degree; mnl->PrecisionHfinal = precision_hfinal;
  mnl->MaxPtildeDegree = NTILDE_CHEBYMAX;
  strncpy(mnl->MDPolyRootsFile, roots_file, sizeof(mnl->MDPolyRootsFile) - 1);
  mnl->rngrepro = 1; mnl->rec_ev = 0;
  mnl->pf = pf; mnl->pf2 = pf2;
  w[0] = w0; w[1] = w1;
  mnl->w_fields = w;
  g_debug_level = debug;
  (void)tmpoly_derivative();
  return init_ndpoly_monomial(0);
}

void tmpoly_set_precision_hfinal(double p) { monomial_list[0].PrecisionHfinal = p; }
int tmpoly_md_degree(void) { return monomial_list[0].MDPolyDegree; }
int tmpoly_ptilde_degree(void) { return monomial_list[0].PtildeDegree; }
double *tmpoly_md_coefs(void) { return monomial_list[0].MDPolyCoefs; }
double *tmpoly_ptilde_coefs(void) { return monomial_list[0].PtildeCoefs; }
double *tmpoly_roots(void) { return (double *)monomial_list[0].MDPolyRoots; }
double tmpoly_evmin(void) { return monomial_list[0].EVMin; }
double tmpoly_evmaxinv(void) { return monomial_list[0].EVMaxInv; }
double tmpoly_energy0(void) { return monomial_list[0].energy0; }
double tmpoly_energy1(void) { return monomial_list[0].energy1; }
double tmpoly_forcefactor(void) { return monomial_list[0].forcefactor; }

void tmpoly_call_derivative(void) { (void)tmpoly_derivative(); ndpoly_derivative(0, &hf); }
/* the heatbath draws its Gaussian field itself (ndpoly_monomial.c:180,184): the same two draws are made first into eta_up / eta_dn from
 * the same generator state, so that the caller knows the field the result belongs to */
void tmpoly_call_heatbath(int seed, spinor *eta_up, spinor *eta_dn) {
  start_ranlux(1, seed);
  random_spinor_field_eo(eta_up, 1, RN_GAUSS);
  random_spinor_field_eo(eta_dn, 1, RN_GAUSS);
  start_ranlux(1, seed);
  (void)tmpoly_derivative();
  ndpoly_heatbath(0, &hf);
}
double tmpoly_call_acc(void) { (void)tmpoly_derivative(); return ndpoly_acc(0, &hf); }
