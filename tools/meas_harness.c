/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_meas.py together with the reference's own meas/correlators.c,
 * meas/pion_norm.c, meas/polyakov_loop.c, meas/oriented_plaquettes.c, source_generation.c and linalg/convert_eo_to_lexic.c
 * (compiled in place into a temporary directory) and oracle/_ref/libtmref.so, which provides the geometry, the fields, RANLUX and
 * the globals.
 *
 * What the two correlator measurements need besides their own file is defined here: measurement_list, operator_list / no_operators
 * with an empty init_operators, an operator whose `inverter` copies a given propagator into prop0 / prop1, and an invert_eo that
 * does the same -- so correlators_measurement and pion_norm_measurement run UNMODIFIED on a known field and write their files.
 * The files hold six digits; the raw per-slice sums in full precision are taken by tmmeas_slice_sums, which is the statements of
 * correlators.c:156-170 / pion_norm.c:95-107 over the reference's own macros and convert_eo_to_lexic. */
#include <stdlib.h>
#include <string.h>
#include <complex.h>
#include "global.h"
#include "su3.h"
#include "su3spinor.h"
#include "operator.h"
#include "invert_eo.h"
#include "linalg/convert_eo_to_lexic.h"
#include "meas/measurements.h"
#include "meas/correlators.h"
#include "meas/pion_norm.h"
#include "meas/polyakov_loop.h"
#include "meas/oriented_plaquettes.h"

measurement measurement_list[max_no_measurements];
int no_measurements = 1;
operator operator_list[max_no_operators];
int no_operators = 0;
int init_operators(void) { return 0; }

static spinor *prop_even = NULL, *prop_odd = NULL;

/* the propagator the stubbed inversions return: two e/o halves, spinor [VOLUME/2] each (copied) */
void tmmeas_set_propagator(const double *even, const double *odd) {
  if (!prop_even) {
    prop_even = malloc(sizeof(spinor) * (VOLUME / 2));
    prop_odd = malloc(sizeof(spinor) * (VOLUME / 2));
  }
  memcpy(prop_even, even, sizeof(spinor) * (VOLUME / 2));
  memcpy(prop_odd, odd, sizeof(spinor) * (VOLUME / 2));
}
static void copy_inverter(const int op_id, const int index_start, const int write_prop) {
  operator *o = &operator_list[op_id];
  (void)index_start; (void)write_prop;
  memcpy(o->prop0, prop_even, sizeof(spinor) * (VOLUME / 2));
  memcpy(o->prop1, prop_odd, sizeof(spinor) * (VOLUME / 2));
}
int invert_eo(spinor *const Even_new, spinor *const Odd_new, spinor *const Even, spinor *const Odd, const double precision,
              const int iter_max, const int solver_flag, const int rel_prec, const int sub_evs_flag, const int even_odd_flag,
              const int no_extra_masses, double *const extra_masses, solver_params_t solver_params, const int id,
              const ExternalInverter external_inverter, const SloppyPrecision sloppy, const CompressionType compression) {
  (void)Even; (void)Odd; (void)precision; (void)iter_max; (void)solver_flag; (void)rel_prec; (void)sub_evs_flag; (void)even_odd_flag;
  (void)no_extra_masses; (void)extra_masses; (void)solver_params; (void)id; (void)external_inverter; (void)sloppy; (void)compression;
  memcpy(Even_new, prop_even, sizeof(spinor) * (VOLUME / 2));
  memcpy(Odd_new, prop_odd, sizeof(spinor) * (VOLUME / 2));
  return 0;
}

static measurement *entry(enum MEAS_TYPE type, int max_source_slice) {
  measurement *m = &measurement_list[0];
  memset(m, 0, sizeof(*m));
  m->type = type; m->initialised = 1; m->id = 0; m->freq = 1;
  m->max_iter = 1; m->seed = 0; m->max_source_slice = max_source_slice; m->all_time_slices = 0; m->no_samples = 1;
  return m;
}
/* correlators_measurement with one TMWILSON operator: writes onlinemeas.<traj> into the working directory */
void tmmeas_correlators(int traj, double kappa, double mu) {
  entry(ONLINE, T)->measurefunc = &correlators_measurement;
  memset(&operator_list[0], 0, sizeof(operator));
  operator_list[0].type = TMWILSON; operator_list[0].kappa = kappa; operator_list[0].mu = mu;
  operator_list[0].inverter = &copy_inverter;
  no_operators = 1;
  correlators_measurement(traj, 0, 0);
}
/* pion_norm_measurement: writes pionnormcorrelator_finiteT.<traj> and appends to pion_norm.data */
void tmmeas_pion_norm(int traj) {
  entry(PIONNORM, LZ)->measurefunc = &pion_norm_measurement;
  pion_norm_measurement(traj, 0, 0);
}
/* raw sums: dir 0 -> pp, pa, p4 [T] (correlators.c:156-170), dir 3 -> pp [LZ] (pion_norm.c:95-107) */
void tmmeas_slice_sums(int dir, double *pp, double *pa, double *p4) {
  int i, j, t, z;
  double res, respa, resp4;
  spinor phi;
  convert_eo_to_lexic(g_spinor_field[DUM_MATRIX], prop_even, prop_odd);
  if (dir == 0) {
    for (t = 0; t < T; t++) {
      j = g_ipt[t][0][0][0];
      res = 0.; respa = 0.; resp4 = 0.;
      for (i = j; i < j + LX * LY * LZ; i++) {
        res += _spinor_prod_re(g_spinor_field[DUM_MATRIX][i], g_spinor_field[DUM_MATRIX][i]);
        _gamma0(phi, g_spinor_field[DUM_MATRIX][i]);
        respa += _spinor_prod_re(g_spinor_field[DUM_MATRIX][i], phi);
        _gamma5(phi, phi);
        resp4 += _spinor_prod_im(g_spinor_field[DUM_MATRIX][i], phi);
      }
      pp[t] = res; pa[t] = respa; p4[t] = resp4;
    }
  } else {
    for (z = 0; z < LZ; z++) {
      res = 0.;
      j = g_ipt[0][0][0][z];
      for (i = 0; i < T * LX * LY; i++) {
        res += _spinor_prod_re(g_spinor_field[DUM_MATRIX][j], g_spinor_field[DUM_MATRIX][j]);
        j += LZ;
      }
      pp[z] = res;
    }
  }
}

int tmmeas_polyakov_loop_dir(int nstore, int dir) { return polyakov_loop_dir(nstore, dir); }
/* polyakov_loop keeps its Kahan accumulators in static variables that it never resets: ONE call per loaded copy of this library */
void tmmeas_polyakov_loop(int mu, double *pl) {
  _Complex double c = 0.0;
  polyakov_loop(&c, mu);
  pl[0] = creal(c); pl[1] = cimag(c);
}
void tmmeas_oriented_plaquettes(double *plaq) { measure_oriented_plaquettes((const su3 **)g_gauge_field, plaq); }
/* appends to oriented_plaquettes.data in the working directory */
void tmmeas_oriented_plaquettes_measurement(int traj) {
  entry(ORIENTED_PLAQUETTES, 0)->measurefunc = &oriented_plaquettes_measurement;
  oriented_plaquettes_measurement(traj, 0, 0);
}
