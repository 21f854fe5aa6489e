/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_rat.py together with the reference's own operator/tm_operators_nd.c and
 * linalg/assign_add_mul.c (compiled in place into a temporary directory) and oracle/_ref/libtmref.so, which provides
 * Hopping_Matrix, the single-flavour operators, the linalg set, deriv_Sb, the geometry and the globals.
 *
 * What tm_operators_nd.c needs and libtmref.so does not define: the phmc globals (phmc.h:29-35) and the helpers of the
 * polynomial code paths that the fixtures never call -- inert dummies, as in tools/nd_harness.c. */
#include <complex.h>
#include <stddef.h>

double phmc_invmaxev = 1.0;
double phmc_Cpol = 1.0;
_Complex double *phmc_root = NULL;
int phmc_dop_n_cheby = 0;
void compact(void *R, void *S, void *P) { (void)R; (void)S; (void)P; }
void decompact(void *S, void *P, void *R) { (void)S; (void)P; (void)R; }

extern double g_mubar, g_epsbar;
void tmrat_set(double mubar, double epsbar, double invmaxev) { g_mubar = mubar; g_epsbar = epsbar; phmc_invmaxev = invmaxev; }

/* the doublet operators use g_spinor_field[DUM_MATRIX .. DUM_MATRIX+5]; oracle/ref_harness.c reserves three fields there */
extern int DUM_MATRIX;
void tmrat_set_dum(int dum) { DUM_MATRIX = dum; }
