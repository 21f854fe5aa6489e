/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_traj.py together with the reference's own monomial/moment_energy.c (and
 * expo.c where oracle/_ref/libtmref.so does not define restoresu3_in_place), compiled in place into a temporary directory, and
 * libtmref.so, which provides VOLUME and the globals.
 *
 * moment_energy is the reference's function.  The three link loops of update_tm.c and the norm loop of monitor_forces.c are not
 * callable functions there: they are written out below on the reference's own macros and restoresu3_in_place, in the serial
 * (non-OpenMP, non-MPI) form, with the lines they restate.  All arrays are the caller's, in the layouts of g_gauge_field
 * ([VOLUME][4] su3) and of hamiltonian_field_t::momenta / ::derivative ([VOLUME][4] su3adj). */
#include <math.h>
#include <stdlib.h>
#include "global.h"
#include "su3.h"
#include "su3adj.h"
#include "expo.h"
#include "monomial/moment_energy.h"

/* moment_energy.c:46-89 on momenta[VOLUME][4] */
double tmtraj_moment_energy(double *mom) {
  su3adj **rows = malloc((size_t)VOLUME * sizeof(su3adj *));
  for (int i = 0; i < VOLUME; i++) rows[i] = (su3adj *)mom + 4 * (size_t)i;
  const double e = moment_energy(rows);
  free(rows);
  return e;
}

/* update_tm.c:115-121: gauge_tmp <- gaugefield */
void tmtraj_snapshot(double *gauge_tmp, const double *gaugefield) {
  const su3 *v;
  su3 *w;
  for (int ix = 0; ix < VOLUME; ix++) {
    for (int mu = 0; mu < 4; mu++) {
      v = (const su3 *)gaugefield + 4 * (size_t)ix + mu;
      w = (su3 *)gauge_tmp + 4 * (size_t)ix + mu;
      _su3_assign(*w, *v);
    }
  }
}

/* update_tm.c:333-339: gaugefield <- gauge_tmp */
void tmtraj_restore(double *gaugefield, const double *gauge_tmp) {
  su3 *v;
  const su3 *w;
  for (int ix = 0; ix < VOLUME; ix++) {
    for (int mu = 0; mu < 4; mu++) {
      v = (su3 *)gaugefield + 4 * (size_t)ix + mu;
      w = (const su3 *)gauge_tmp + 4 * (size_t)ix + mu;
      _su3_assign(*v, *w);
    }
  }
}

/* update_tm.c:321-326 */
void tmtraj_reunitarize(double *gaugefield) {
  su3 *v;
  for (int ix = 0; ix < VOLUME; ix++) {
    for (int mu = 0; mu < 4; mu++) {
      v = (su3 *)gaugefield + 4 * (size_t)ix + mu;
      restoresu3_in_place(v);
    }
  }
}

/* update_tm.c:233-272, one thread, one rank: ret_gauge_diff */
double tmtraj_gauge_diff(const double *gaugefield, const double *gauge_tmp) {
  const su3 *v, *w;
  su3 v0;
  double ds, tt, tr, ts, ks = 0., kc = 0.;
  for (int ix = 0; ix < VOLUME; ++ix) {
    for (int mu = 0; mu < 4; ++mu) {
      v = (const su3 *)gaugefield + 4 * (size_t)ix + mu;
      w = (const su3 *)gauge_tmp + 4 * (size_t)ix + mu;
      _su3_minus_su3(v0, *v, *w);
      _su3_square_norm(ds, v0);
      tr = sqrt(ds) + kc;
      ts = tr + ks;
      tt = ts - ks;
      ks = ts;
      kc = tr - tt;
    }
  }
  kc = ks + kc;
  return kc;
}

/* monitor_forces.c:64-82, one thread, one rank */
void tmtraj_force_norms(const double *derivative, double *sum_out, double *max_out) {
  double sum = 0., max = 0., sum2;
  for (int i = 0; i < VOLUME; i++) {
    for (int mu = 0; mu < 4; mu++) {
      const su3adj *d = (const su3adj *)derivative + 4 * (size_t)i + mu;
      sum2 = _su3adj_square_norm(*d);
      sum += sum2;
      if (sum2 > max) max = sum2;
    }
  }
  *sum_out = sum;
  *max_out = max;
}
