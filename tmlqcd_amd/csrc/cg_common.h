// What the device-resident CG solvers of cg.hip (single flavour) and nd32.hip (the doublet's rg_mixed_cg_her_nd) share: the state
// block with its scalar step, the sum + scalar kernel of a single rank, the inner loop of the reliable-update solvers and their
// restart logic.  The solvers differ in the field updates of an iteration and in the fields themselves, nothing else.
#pragma once
#include "tmhip_internal.h"

static inline v4f *F4(tmhip_field *f) { return reinterpret_cast<v4f *>(f->d32); }   // fp32 field as six float4 planes

struct CgState {
  double normsq, pro, err, alpha, beta, squarenorm, eps_sq;
  int rel_prec, done, iters, it;
  // inner loop of mixed_cg_her (mixed_cg_her.c:141): stop when err <= innereps * sqnrm_outer, after max_inner
  // iterations, or when 1.3 err already meets the outer target
  int inner; int max_inner; double innereps, sqnrm_outer;
  // inner loops of rg_mixed_cg_her (rg_mixed_cg_her.c:74-176), inner = 2 (float scalars) / 3 (double scalars):
  // run while rho > delta * rhomax and iter_base + j <= max_total; leave early when 1.3 rho < eps_sq
  double delta, rhomax; int iter_base, max_total;
  // fused Qtm_pm_psi iteration: alpha is known (and P += alpha p still owed) between the two scalar updates
  int x_pending;
};

// two copies of the state (the self-summing small-lattice iteration reads one and writes the other) and {pro, alpha} of the running iteration
static int cg_state_alloc(tmhip_ctx *ctx) {
  if (ctx->cg_state) return 0;
  TMHIP_CHECK(hipMalloc(&ctx->cg_state, 2 * sizeof(CgState) + 2 * sizeof(double)));
  TMHIP_CHECK(hipMemsetAsync(ctx->cg_state, 0, 2 * sizeof(CgState) + 2 * sizeof(double), ctx->stream));
  return 0;
}

// one partial per block, blocks numbered x fastest (gridDim.z > 1: the two flavours of a doublet)
__device__ __forceinline__ void cg_block_reduce_store(double v, double *partials) {
  __shared__ double wsum[LA_BS / 64];
  v = tmhip_wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_BS / 64; k++) s += wsum[k];
    partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
  }
}

// The field kernels are written once for both precisions: V = v2d (fp64 field, twelve planes of complex doubles) or v4f (fp32
// field, six planes of component pairs); scalars have the element type, sums are accumulated in double.
__device__ __forceinline__ double la_dot(v2d a, v2d b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ double la_dot(v4f a, v4f b) { return ((double)a.x * b.x + (double)a.y * b.y) + ((double)a.z * b.z + (double)a.w * b.w); }

#define CG_SUM_BS 1024   // one block; the fused stencils deliver one partial per wave (8192 at 32^4), so use the widest block

// WHICH 0: after the dot  -> alpha = normsq / pro            (cg_her.c:93-94)
// WHICH 1: after |sf0|^2  -> stopping test, beta, normsq      (cg_her.c:101-126)
template <int WHICH>
__device__ __forceinline__ void cg_scalar_update(CgState *st, const double *sum, double *hist, int hist_len) {
  if (WHICH == 0) {
    st->pro = *sum;
    if (st->inner == 2 || st->inner == 1) st->alpha = (double)((float)st->normsq / (float)st->pro);   // float pro, alpha_cg: rg_mixed_cg_her.c:126, mixed_cg_her.c:67-69,127-128
    else st->alpha = st->normsq / st->pro;
    st->x_pending = 1;
  } else if (st->inner >= 2) {
    st->it += 1;
    bool stop;
    if (st->inner == 2) {          // rg_mixed_cg_her.c:122-145, scalars in float like the reference
      const float rho = (float)*sum, eps = (float)st->eps_sq, delta = (float)st->delta;
      float rhomax = (float)st->rhomax;
      st->err = rho;
      st->beta = (double)(rho / (float)st->normsq);
      st->normsq = rho;
      stop = 1.3 * rho < eps;
      if (!stop) {
        if (rho > rhomax) rhomax = rho;
        st->rhomax = rhomax;
        stop = !(rho > delta * rhomax && st->it + st->iter_base <= st->max_total);
      }
    } else {                       // inner_loop_high, rg_mixed_cg_her.c:74-108
      const double rho = *sum;
      st->err = rho;
      st->beta = rho / st->normsq;
      st->normsq = rho;
      stop = 1.3 * rho < st->eps_sq;
      if (!stop) {
        if (rho > st->rhomax) st->rhomax = rho;
        stop = !(rho > st->delta * st->rhomax && st->it + st->iter_base <= st->max_total);
      }
    }
    if (stop) { st->done = 1; st->iters = st->it; }
  } else {
    const double err = st->inner ? (double)(float)*sum : *sum;   // mixed_cg_her.c:67-69: err, beta_cg, sqnrm2 are floats in the inner loop
    st->err = err;
    st->it += 1;
    if (hist && st->it - 1 < hist_len) hist[st->it - 1] = err;
    bool conv;
    if (st->inner)
      conv = (err <= st->innereps * st->sqnrm_outer) || (st->it - 1 == st->max_inner) ||
             ((1.3 * err <= st->eps_sq) && (st->rel_prec == 0)) || ((1.3 * err <= st->eps_sq * st->squarenorm) && (st->rel_prec == 1));
    else
      conv = ((err <= st->eps_sq) && (st->rel_prec == 0)) || ((err <= st->eps_sq * st->squarenorm) && (st->rel_prec == 1));
    if (conv) { st->done = 1; st->iters = st->it; }
    else { st->beta = st->inner ? (double)((float)err / (float)st->normsq) : err / st->normsq; st->normsq = err; }
  }
}

// single rank: the fixed-order sum of the partials and the scalar update in one launch (no all-reduce in between)
template <int WHICH>
__global__ __launch_bounds__(CG_SUM_BS) void cg_sum_scalar_kernel(const double *__restrict__ partials, int n, double *out, CgState *st, double *hist,
                                                                  int hist_len) {
  // The state is fetched into LDS by the last wave while the others are already loading partials: the scalar update then works
  // on LDS instead of walking a chain of dependent global loads (done, inner, normsq, ...) after the reduction.
  static_assert(sizeof(CgState) % sizeof(double) == 0 && sizeof(CgState) / sizeof(double) <= 64, "CgState is copied as doubles by one wave");
  constexpr int NW = sizeof(CgState) / sizeof(double);
  __shared__ CgState ls;
  __shared__ double sm[CG_SUM_BS / 64];
  const int lw = (int)threadIdx.x - (CG_SUM_BS - 64);
  if (lw >= 0 && lw < NW) reinterpret_cast<double *>(&ls)[lw] = reinterpret_cast<const double *>(st)[lw];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += CG_SUM_BS) acc += partials[i];
  acc = tmhip_wave_sum(acc);                       // fixed order: strided per-lane sums, butterfly per wave, then the 16 wave sums
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (ls.done) { if (WHICH == 0 && threadIdx.x == 0) st->x_pending = 0; return; }   // block-uniform
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < CG_SUM_BS / 64; w++) tot += sm[w];
    *out = tot;
    cg_scalar_update<WHICH>(&ls, &tot, hist, hist_len);
  }
  __syncthreads();
  if (lw >= 0 && lw < NW) reinterpret_cast<double *>(st)[lw] = reinterpret_cast<const double *>(&ls)[lw];
}

// ------------------------------------------------------------------ reliable-update mixed CG
// inner_loop / inner_loop_high of rg_mixed_cg_her.c:74-176 and of rg_mixed_cg_her_nd.c:75-154 (non-pipelined, Fletcher-Reeves beta):
// returns j, updates *rho1.  enqueue(st) puts one iteration on ctx->stream; its scalar steps run on `st` with inner = 2 (fp32) / 3.
template <class Enqueue>
static int rg_inner_loop(tmhip_ctx *ctx, const char *who, bool fp32, double *rho1, double delta, double eps_sq, int iter_base, int max_iter, int *j_out,
                         Enqueue enqueue) {
  CgState *st = (CgState *)ctx->cg_state;
  CgState h;
  memset(&h, 0, sizeof(h));
  h.normsq = *rho1; h.rhomax = *rho1; h.delta = delta; h.eps_sq = eps_sq;
  h.inner = fp32 ? 2 : 3; h.iter_base = iter_base; h.max_total = max_iter;
  *j_out = 0;
  // the reference tests the loop condition before the first iteration as well (rho = rhomax => rho > delta rhomax iff delta < 1)
  const bool enter = fp32 ? ((float)*rho1 > (float)delta * (float)*rho1) : (*rho1 > delta * *rho1);
  if (!enter || iter_base > max_iter) return 0;
  TMHIP_CHECK(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  const int batch = ctx->opt_cg_batch > 0 ? ctx->opt_cg_batch : 4;
  const double t_rel = delta * *rho1, t_abs = eps_sq / 1.3;      // the two exits of rg_mixed_cg_her.c:122-145 (rhomax >= rho1)
  const double tgt = t_rel > t_abs ? t_rel : t_abs;              // as in tmhip_mixed_cg_her: poll every iteration close to the restart
  // runs until `done`; the device-side test counts against max_iter itself, so more than max_iter + batch enqueued iterations is a failure
  if (tmhip_poll_loop(ctx, max_iter + batch, false, batch, 1.0e3 * tgt, &st->done, &st->err, 0, true, [&](int) { return enqueue(st); })) return 1;
  TMHIP_CHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (!h.done) TMHIP_FAIL("%s: inner loop did not terminate", who);
  *j_out = h.iters;
  *rho1 = h.normsq;
  return 0;
}

/* solver/rg_mixed_cg_her.c:180-347 and solver/rg_mixed_cg_her_nd.c:189-341, which is the same text on pairs of fields.  fp32 CG with
 * true reliable updates: the inner loop runs until the iterated residual has dropped by `delta` relative to its maximum since the last
 * update, then the solution is accumulated and the residual recomputed in fp64; when the outer-iteration estimate N_outer is nearly
 * used up the solver falls back to fp64 inner loops.  *iters: the reference's count iter_out + iter_in_sp + iter_in_dp, or -1.
 * F names the fields and their operations, each returning non-zero on failure:
 *   source_norm(&s)            s = |Q|^2
 *   start()                    x = 0 (fp32), P = 0, phigh = rhigh = Q
 *   rhigh_norm(&s)             s = |rhigh|^2
 *   restart32()                r = p = (float) rhigh                      (assign_to_32; assign_32(p, r) is the same rounding of the same source)
 *   zero_x32()
 *   loop32(&rho, delta, eps, base, max_iter, &j) / loop64(..)             rg_inner_loop on (x, p, q, r) / (xhigh, phigh, qhigh, rhigh)
 *   accumulate32()             P += x                                     (addto_32)
 *   true_residual(&s)          qhigh = A P, rhigh = Q - qhigh, s = |rhigh|^2
 *   restart64()                phigh = rhigh, xhigh = 0
 *   accumulate64()             P += xhigh */
template <class F>
static int rg_mixed_solve(F &f, int max_iter, double eps_sq, int rel_prec, double delta_in, int *iters, int *iter_out_p, int *iter_sp_p,
                          int *iter_dp_p) {
  const float delta = (float)delta_in;                                /* :185 */
  int iter_in_sp = 0, iter_in_dp = 0, iter_out = 0, high_control = 0, j;
  double rho_dp, sourcesquarenorm, target_eps_sq;
  float rho_sp;
  if (f.source_norm(&sourcesquarenorm)) return 1;
  target_eps_sq = rel_prec == 1 ? eps_sq * sourcesquarenorm : eps_sq;  /* :225-232 */
  const int N_outer = (int)ceil(log10(sourcesquarenorm * delta / target_eps_sq));   /* :236 */
  if (f.start()) return 1;
  if (f.rhigh_norm(&rho_dp)) return 1;
  if (f.restart32()) return 1;
  rho_sp = (float)rho_dp;
#define RG_SP_LOOP()                                                                                                   \
  do {                                                                                                                 \
    double rho1 = rho_sp;                                                                                              \
    if (f.loop32(&rho1, delta, (double)(float)target_eps_sq, iter_out + iter_in_sp + iter_in_dp, max_iter, &j)) return 1; \
    rho_sp = (float)rho1; iter_in_sp += j;                                                                             \
  } while (0)
#define RG_RETURN(val)                                                                                                 \
  do {                                                                                                                 \
    *iters = (val);                                                                                                    \
    if (iter_out_p) *iter_out_p = iter_out;                                                                            \
    if (iter_sp_p) *iter_sp_p = iter_in_sp;                                                                            \
    if (iter_dp_p) *iter_dp_p = iter_in_dp;                                                                            \
    return 0;                                                                                                          \
  } while (0)
  RG_SP_LOOP();
  for (iter_out = 1; iter_out < N_outer; ++iter_out) {
    if (high_control == 0) {                                           /* :260-269 */
      if (f.accumulate32()) return 1;
      if (f.true_residual(&rho_dp)) return 1;
    }
    if (high_control == 1) {                                           /* :272-286 double precision fail-safe */
      if (f.restart64()) return 1;
      if (f.loop64(&rho_dp, delta, target_eps_sq, iter_out + iter_in_sp + iter_in_dp, max_iter, &j)) return 1;
      iter_in_dp += j;
      rho_sp = (float)rho_dp;
      if (f.accumulate64()) return 1;                                  /* add(P, P, xhigh) */
      if (f.true_residual(&rho_dp)) return 1;
    }
    const int total = iter_in_sp + iter_in_dp + iter_out;
    if (rho_dp <= target_eps_sq || total >= max_iter) RG_RETURN(total >= max_iter ? -1 : total);   /* :294-307 */
    if (iter_out >= N_outer - 2) {                                     /* :310-313 */
      high_control = 1;
      continue;
    }
    if (f.restart32()) return 1;                                       /* :315-318 */
    rho_sp = (float)rho_dp;
    if (f.zero_x32()) return 1;
    RG_SP_LOOP();
  }
  RG_RETURN(-1);                                                       /* :326-330 convergence failure */
#undef RG_SP_LOOP
#undef RG_RETURN
}
