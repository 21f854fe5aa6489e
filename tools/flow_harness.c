/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_flow.py together with the reference's own meas/gradient_flow.c,
 * meas/measure_clover_field_strength_observables.c, matrix_utils.c, get_staples.c, measure_gauge_action.c and aligned_malloc.c
 * (compiled in place into a temporary directory) and oracle/_ref/libtmref.so, which provides the geometry, g_gauge_field and the
 * globals.
 *
 * measurement_list (meas/measurements.h) is defined and filled here so that the Python side need not mirror its layout, and
 * GaugeInfo because measure_gauge_action.c stores the plaquette energy there. */
#include <stdlib.h>
#include <string.h>
#include "global.h"
#include "su3.h"
#include "io/params.h"
#include "aligned_malloc.h"
#include "gettime.h"
#include "measure_gauge_action.h"
#include "meas/field_strength_types.h"
#include "meas/measurements.h"
#include "meas/gradient_flow.h"
#include "meas/measure_clover_field_strength_observables.h"

measurement measurement_list[max_no_measurements];
int no_measurements = 1;
paramsGaugeInfo GaugeInfo;

static aligned_su3_field_t vt, x1, x2, z;
static int live = 0;

/* as gradient_flow_measurement does (gradient_flow.c:162-170) */
void tmflow_begin(void) {
  if (!live) {
    vt = aligned_su3_field_alloc(VOLUMEPLUSRAND + g_dbw2rand);
    x1 = aligned_su3_field_alloc(VOLUMEPLUSRAND + g_dbw2rand);
    x2 = aligned_su3_field_alloc(VOLUMEPLUSRAND + g_dbw2rand);
    z = aligned_su3_field_alloc(VOLUME);
    live = 1;
  }
  memcpy(vt.field[0], g_gauge_field[0], sizeof(su3) * 4 * (VOLUMEPLUSRAND + g_dbw2rand));
}
void tmflow_step(double eps) { step_gradient_flow(vt.field, x1.field, x2.field, z.field, 0, eps); }
/* out: su3 [VOLUME][4] */
void tmflow_links(double *out) { memcpy(out, vt.field[0], sizeof(su3) * 4 * VOLUME); }
static void obs(su3 **f, double *peq) {
  field_strength_obs_t fso;
  measure_clover_field_strength_observables((const su3 **)f, &fso);
  peq[0] = measure_plaquette((const su3 **)f) / (6.0 * VOLUME * g_nproc);
  peq[1] = fso.E;
  peq[2] = fso.Q;
}
/* peq[3] = P, E, Q of the flowed field / of g_gauge_field */
void tmflow_observables(double *peq) { obs(vt.field, peq); }
void tmflow_observables_resident(double *peq) { obs(g_gauge_field, peq); }
/* the reference's measurement with measurement_list[0] as a GRADIENT_FLOW entry: writes gradflow.<traj> into the working directory */
void tmflow_measurement(int traj, double eps, double tmax) {
  measurement *m = &measurement_list[0];
  memset(m, 0, sizeof(*m));
  m->type = GRADIENT_FLOW; m->initialised = 1; m->id = 0; m->freq = 1;
  m->gf_eps = eps; m->gf_tmax = tmax;
  m->measurefunc = &gradient_flow_measurement;
  gradient_flow_measurement(traj, 0, 0);
}
/* the cost of the reference's own flow: nsteps of step_gradient_flow + the two measures, seconds (gettime.c) */
double tmflow_time(double eps, int nsteps) {
  double peq[3];
  tmflow_begin();
  const double t0 = gettime();
  for (int i = 0; i < nsteps; i++) { tmflow_step(eps); tmflow_observables(peq); }
  return gettime() - t0;
}
