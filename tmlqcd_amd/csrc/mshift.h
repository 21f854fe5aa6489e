// The multi-shift CG recurrences (solver/cg_mms_tm.c:122-189, solver/cg_mms_tm_nd.c:126-201), written once for the doublet
// solvers (nd.hip) and the single-flavour solver (mms.hip): device-side state, the alpha step and the beta step.  The CG runs
// on shift 0; shift s >= 1 rides along with the relative sigma[s] = shifts[s]^2 - shifts[0]^2.  Each solver keeps its own
// one-block alpha / beta kernels, which do their fixed-order sums and hand the totals to thread 0's call of the steps below,
// and its own field kernels, which read the coefficients from the state.
#pragma once
#include "tmhip_internal.h"

#define MSHIFT_MAX_SHIFTS 32
struct MshiftState {
  double alpha0, sigma0;     // alpha0 repeats alphas[0]; adjacent: the _RSH stencil epilogue reads {alpha0, sigma0} through one pointer
  double normsq, err, target, eps_sq;   // eps_sq: the absolute threshold of the shift drop
  int it, done, done_it, conv;          // iterations run; the stopping test fired, in iteration done_it, and it was err <= target
  int active, pact, max_iter, pad;      // pact: shifts active when the iteration began (a dropped shift's P is updated once more)
  // [0]: the CG's own alpha and beta (sigma[0], zita[0], zitam1[0] unused)
  double sigma[MSHIFT_MAX_SHIFTS], zita[MSHIFT_MAX_SHIFTS], zitam1[MSHIFT_MAX_SHIFTS], alphas[MSHIFT_MAX_SHIFTS], betas[MSHIFT_MAX_SHIFTS];
};

// alphas[0] = normsq / pro and the zita / alphas recurrences of the shifts still active (cg_mms_tm.c:125-140, cg_mms_tm_nd.c:126-146).
// pro = <p, (A + sigma0) p>.  Called by one thread, not after `done`.
__device__ __forceinline__ void mshift_alpha_step(MshiftState *st, double pro) {
  const double alpham1 = st->alphas[0];
  const double a0 = st->normsq / pro;
  st->alphas[0] = a0;
  st->alpha0 = a0;
  const double b0 = st->betas[0];   // the previous iteration's beta (0 at the start)
  for (int im = 1; im < st->active; im++) {
    const double gamma = st->zita[im] * alpham1 / (a0 * b0 * (1. - st->zita[im] / st->zitam1[im]) + alpham1 * (1. + st->sigma[im] * a0));
    st->zitam1[im] = st->zita[im];
    st->zita[im] = gamma;
    st->alphas[im] = a0 * st->zita[im] / st->zitam1[im];
  }
}

// Shift drop (cg_mms_tm.c:146-153, cg_mms_tm_nd.c:158-167: new alphas, not yet updated ps; sn = |ps_last|^2, looked at on a check
// iteration only), stopping test (:170-176 / :186-190; iteration max_iter - 1 is the last one) and betas (:180-189 / :195-201).
// err = |r|^2.  Called by one thread, not after `done`.
__device__ __forceinline__ void mshift_beta_step(MshiftState *st, double err, double sn, int check, int iteration) {
  st->pact = st->active;
  if (check && st->active > 1) {
    const double al = st->alphas[st->active - 1];
    if (al * al * sn <= st->eps_sq) st->active -= 1;
  }
  st->err = err;
  st->it = iteration + 1;
  const bool conv = err <= st->target;
  if (conv || iteration == st->max_iter - 1) { st->done = 1; st->done_it = iteration; st->conv = conv; return; }
  const double b0 = err / st->normsq;
  st->betas[0] = b0;
  st->normsq = err;
  for (int im = 1; im < st->active; im++) st->betas[im] = b0 * st->zita[im] * st->alphas[im] / (st->zitam1[im] * st->alphas[0]);
}
