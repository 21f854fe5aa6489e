/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_gauge.py together with the reference's own monomial/gauge_monomial.c,
 * get_staples.c, get_rectangle_staples.c, measure_gauge_action.c and measure_rectangles.c (compiled in place into a temporary
 * directory) and oracle/_ref/libtmref.so, which provides the geometry, g_gauge_field and the globals (g_beta, ...).
 *
 * monomial (monomial/monomial.h) is filled here so that the Python side need not mirror its layout. */
#include <stdlib.h>
#include "global.h"
#include "su3.h"
#include "su3adj.h"
#include "io/params.h"
#include "hamiltonian_field.h"
#include "monomial/monomial.h"
#include "monomial/gauge_monomial.h"
#include "measure_gauge_action.h"
#include "measure_rectangles.h"

monomial monomial_list[max_no_monomials];
paramsGaugeInfo GaugeInfo;

static su3adj **rows = NULL;
static void fill(hamiltonian_field_t *hf, double *df) {
  if (!rows) rows = malloc((size_t)VOLUMEPLUSRAND * sizeof(su3adj *));
  for (int i = 0; i < VOLUMEPLUSRAND; i++) rows[i] = (su3adj *)df + 4 * (size_t)i;
  hf->gaugefield = g_gauge_field; hf->momenta = NULL; hf->derivative = rows; hf->update_gauge_copy = 0; hf->traj_counter = 0;
}
void tmgauge_setup(double beta, double c0, double c1, int use_rectangles, double glambda) {
  monomial *m = &monomial_list[0];
  __builtin_memset(m, 0, sizeof(*m));
  g_beta = beta;
  m->c0 = c0; m->c1 = c1; m->use_rectangles = use_rectangles; m->glambda = glambda;
}
/* df: su3adj [VOLUMEPLUSRAND][4], accumulated into; em != 0: gauge_EMderivative */
void tmgauge_derivative(int em, double *df) {
  hamiltonian_field_t hf;
  fill(&hf, df);
  if (em) gauge_EMderivative(0, &hf); else gauge_derivative(0, &hf);
}
double tmgauge_heatbath(void) {
  hamiltonian_field_t hf;
  hf.gaugefield = g_gauge_field; hf.momenta = NULL; hf.derivative = NULL; hf.update_gauge_copy = 0; hf.traj_counter = 0;
  gauge_heatbath(0, &hf);
  return monomial_list[0].energy0;
}
double tmgauge_c0(void) { return monomial_list[0].c0; }
double tmgauge_plaquette(void) { return measure_plaquette((const su3 **)g_gauge_field); }
double tmgauge_action(double lambda) { return measure_gauge_action((const su3 **)g_gauge_field, lambda); }
double tmgauge_plaquette_energy(void) { return GaugeInfo.plaquetteEnergy; }
double tmgauge_rectangles(void) { return measure_rectangles((const su3 **)g_gauge_field); }
