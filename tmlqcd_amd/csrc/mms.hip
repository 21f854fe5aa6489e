// The single-flavour multi-shift CG (solver/cg_mms_tm.c:65-197) on the device: the solves of the rat / ratcor monomials
// (M_psi = Qtm_pm_psi or Qsw_pm_psi on VOLUME/2 sites, solver/monomial_solve.c:176-215) and of the multi-mass propagators of
// invert_eo.c:463-490 (M_psi = Q_pm_psi on VOLUME sites, g_mu = 0).
//
// cg_mms_tm.c solves (M_psi + shifts[s]^2) P_s = Q for all s at once: the CG runs on M_psi + sigma0 (sigma0 = shifts[0]^2 is
// ADDED to the operator, :88,115-118), the other shifts ride along with relative sigma_s = shifts[s]^2 - sigma0 through the
// zita / alphas / betas recurrences (:122-140, :180-189).  One iteration here (e/o operators, cg_her's fusable shapes):
//   s1 = A_-^-1 H_eo p ; s0 = Q_- p, partials of |Q_- p|^2            stencils 1, 2 (cg_enqueue_fused_qtm's, NRM epilogue)
//   pro = |Q_- p|^2 + sigma0 |p|^2 ; alpha0 ; zita_s, alphas_s          one block (|p|^2: left by the previous vector pass)
//   s1 = A_+^-1 H_eo s0 ; r -= alpha0 (Q_+ s0 + sigma0 p), |r|^2       stencils 3, 4 (the _RSH epilogue, A p never stored)
//   shift drop, stopping test, beta0, betas_s                          one block
//   P0 += alpha0 p ; p = r + beta0 p ; P_s += alphas_s ps_s ;          ONE vector pass over every active shift, r read once
//   ps_s = zita_s r + betas_s ps_s ; partials of |p|^2 (and of |ps_last|^2 before a drop check)
// The P_s updates the reference does at :141 are deferred to the vector pass of the same iteration: nothing reads P_s in
// between, and the pass knows which shifts were active when the reference updated them (`pact`: the dropped shift's P
// HAS been updated in its last iteration, :146-153).  Other shapes take the unfused form (operator, then <p, A p> in a kernel
// of its own, then the residual update in a kernel of its own), and Q_pm_psi on FULL fields is the composite of
// tm_operators.c:380-388 over D_psi and gamma5 with the same passes over both halves.  All coefficients live in a MshiftState
// (mshift.h: the state and the recurrences, shared with nd.hip); the host polls `done` between batches only (tmhip_poll_loop,
// tmhip_internal.h).  Every sum is in fixed order (per-wave partials, one-block sums): bitwise reproducible from run to run.
#include "mshift.h"

namespace {

__device__ __forceinline__ double mms_dot(v2d a, v2d b) { return a.x * b.x + a.y * b.y; }

// pro = <p, M p> + sigma0 |p|^2 (cg_mms_tm.c:115-118), then the alpha step
__global__ __launch_bounds__(256) void mms_alpha_kernel(MshiftState *st, const double *part_pro, int n_pro, const double *part_pp, int n_pp) {
  __shared__ double ws[4];
  const double pro_m = tmhip_block_sum256(part_pro, n_pro, ws);
  __syncthreads();
  const double pp = tmhip_block_sum256(part_pp, n_pp, ws);
  if (threadIdx.x != 0 || st->done) return;
  mshift_alpha_step(st, pro_m + st->sigma0 * pp);
}

// |r|^2 and, on a check iteration, |ps_last|^2, then the beta step
__global__ __launch_bounds__(256) void mms_beta_kernel(MshiftState *st, const double *part_r, int n_r, const double *part_sn, int n_sn, int check,
                                                       int iteration) {
  __shared__ double ws[4];
  const double err = tmhip_block_sum256(part_r, n_r, ws);
  __syncthreads();
  const double sn = check ? tmhip_block_sum256(part_sn, n_sn, ws) : 0.0;
  if (threadIdx.x != 0 || st->done) return;
  mshift_beta_step(st, err, sn, check, iteration);
}

// The vector pass.  tab[2 s] = P_s, tab[2 s + 1] = ps_s (s >= 1).  Runs in the iteration that set `done` (then only the P updates,
// :164-165 and :141 of the last iteration) and never after it.  blockIdx.y: the half of a FULL field (one-parity fields: 0 only).
// One partial per wave of |p|^2 (the next alpha kernel's sigma0 |p|^2) and, when sn_next, of |ps_last|^2 (the next drop check).
__global__ __launch_bounds__(256) void mms_vec_kernel(const MshiftState *st, v2d *const *tab, v2d *__restrict__ P0, v2d *__restrict__ p,
                                                      const v2d *__restrict__ r, int ns, int N, double *part_pp, double *part_sn, int sn_next,
                                                      int iteration) {
  const int done = st->done;
  if (done && st->done_it != iteration) return;   // grid-uniform
  const bool fin = done != 0;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const size_t off = (size_t)blockIdx.y * 12 * ns;
  const int pact = st->pact, act = st->active;
  double dpp = 0.0, dsn = 0.0;
  if (i < N) {
    const double a0 = st->alpha0, b0 = st->betas[0];
    v2d rv[12];
    if (!fin) {
#pragma unroll
      for (int c = 0; c < 12; c++) rv[c] = r[off + (size_t)c * ns + i];
    }
    {
      v2d pv[12], xv[12];
#pragma unroll
      for (int c = 0; c < 12; c++) { const size_t o = off + (size_t)c * ns + i; pv[c] = p[o]; xv[c] = P0[o]; }
#pragma unroll
      for (int c = 0; c < 12; c++) {
        const size_t o = off + (size_t)c * ns + i;
        P0[o] = xv[c] + a0 * pv[c];                       // cg_mms_tm.c:164
        if (!fin) {
          const v2d pn = b0 * pv[c] + rv[c];              // :181
          p[o] = pn;
          dpp += mms_dot(pn, pn);
        }
      }
    }
    for (int s = 1; s < pact; s++) {
      v2d *__restrict__ X = tab[2 * s];
      v2d *__restrict__ Ps = tab[2 * s + 1];
      const double al = st->alphas[s], be = st->betas[s], ze = st->zita[s];
      const bool upd = !fin && s < act, last = sn_next && s == act - 1;
      v2d sv[12], xv[12];
#pragma unroll
      for (int c = 0; c < 12; c++) { const size_t o = off + (size_t)c * ns + i; sv[c] = Ps[o]; xv[c] = X[o]; }
#pragma unroll
      for (int c = 0; c < 12; c++) {
        const size_t o = off + (size_t)c * ns + i;
        X[o] = xv[c] + al * sv[c];                        // :141
        if (upd) {
          const v2d nv = be * sv[c] + ze * rv[c];         // :188 (assign_mul_add_mul_r)
          Ps[o] = nv;
          if (last) dsn += mms_dot(nv, nv);
        }
      }
    }
  }
  if (fin) return;
  const int slot = (blockIdx.y * gridDim.x + blockIdx.x) * 4 + (int)(threadIdx.x >> 6);
  tmhip_wave_partial(dpp, part_pp, slot);
  if (sn_next) tmhip_wave_partial(dsn, part_sn, slot);
}

// unfused forms: partials of <p, A p> (the operator's part of pro) ...
__global__ __launch_bounds__(256) void mms_dot_kernel(const MshiftState *st, const v2d *__restrict__ p, const v2d *__restrict__ ap, int ns, int N,
                                                      double *partials) {
  if (st->done) return;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const size_t off = (size_t)blockIdx.y * 12 * ns;
  double d = 0.0;
  if (i < N) {
#pragma unroll
    for (int c = 0; c < 12; c++) { const size_t o = off + (size_t)c * ns + i; d += mms_dot(p[o], ap[o]); }
  }
  tmhip_wave_partial(d, partials, (blockIdx.y * gridDim.x + blockIdx.x) * 4 + (int)(threadIdx.x >> 6));
}

// ... and r -= alpha0 (A p + sigma0 p) with the partials of |r|^2 (cg_mms_tm.c:115-118,166)
__global__ __launch_bounds__(256) void mms_res_kernel(const MshiftState *st, v2d *__restrict__ r, const v2d *__restrict__ ap, const v2d *__restrict__ p,
                                                      int ns, int N, double *partials) {
  if (st->done) return;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const size_t off = (size_t)blockIdx.y * 12 * ns;
  const double a0 = st->alpha0, s0 = st->sigma0;
  double d = 0.0;
  if (i < N) {
#pragma unroll
    for (int c = 0; c < 12; c++) {
      const size_t o = off + (size_t)c * ns + i;
      const v2d rn = r[o] - a0 * (ap[o] + s0 * p[o]);
      r[o] = rn;
      d += mms_dot(rn, rn);
    }
  }
  tmhip_wave_partial(d, partials, (blockIdx.y * gridDim.x + blockIdx.x) * 4 + (int)(threadIdx.x >> 6));
}
}  // namespace

// ---------------------------------------------------------------- host side
struct TmhipMms {
  tmhip_field *w[2][3];                      // [kind][r, p, A p]
  tmhip_field *ps[2][MSHIFT_MAX_SHIFTS];     // [kind][s - 1]: shifted directions (allocated as needed)
  tmhip_field *full_tmp;                     // FULL scratch of Q_pm_psi (g_spinor_field[DUM_MATRIX] of tm_operators.c:383)
  int nps[2];
  double *partials; int max_partials;        // [4][max_partials]: pro, |r|^2, |p|^2, |ps_last|^2
  MshiftState *st;
  v2d **tab;
  int form;                                  // form of the last solve: 0 fused e/o, 1 unfused e/o, 2 FULL composite
};

void tmhip_mms_destroy(tmhip_ctx *ctx) {
  TmhipMms *m = (TmhipMms *)ctx->mms;
  if (!m) return;
  for (int k = 0; k < 2; k++) {
    for (int j = 0; j < 3; j++) tmhip_field_free(ctx, m->w[k][j]);
    for (int j = 0; j < m->nps[k]; j++) tmhip_field_free(ctx, m->ps[k][j]);
  }
  tmhip_field_free(ctx, m->full_tmp);
  if (m->partials) (void)hipFree(m->partials);
  if (m->st) (void)hipFree(m->st);
  if (m->tab) (void)hipFree(m->tab);
  delete m;
  ctx->mms = nullptr;
}

static int mms_prepare(tmhip_ctx *ctx) {
  if (ctx->mms) return 0;
  TmhipMms *m = new TmhipMms();
  ctx->mms = m;
  m->max_partials = 4 * ((2 * ctx->Vh + 255) / 256) + 64;   // one per wave of a vector-pass grid over a FULL field
  TMHIP_CHECK(hipMalloc((void **)&m->partials, (size_t)4 * m->max_partials * sizeof(double)));
  TMHIP_CHECK(hipMemsetAsync(m->partials, 0, (size_t)4 * m->max_partials * sizeof(double), ctx->stream));
  TMHIP_CHECK(hipMalloc((void **)&m->st, sizeof(MshiftState)));
  TMHIP_CHECK(hipMalloc((void **)&m->tab, (size_t)2 * MSHIFT_MAX_SHIFTS * sizeof(v2d *)));
  return 0;
}

// Q_pm_psi (tm_operators.c:380-388) on FULL fields: D_psi at -mu, gamma5, D_psi at +mu, gamma5.  Row TMHIP_OP_Q_PM_FULL of the operator
// table; its FULL scratch field lives with the state of the only solver that takes the row.
int tmhip_Q_pm_psi(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k) {
  if (mms_prepare(ctx)) return 1;
  TmhipMms *m = (TmhipMms *)ctx->mms;
  if (!m->full_tmp && tmhip_field_alloc(ctx, TMHIP_FIELD_FULL, &m->full_tmp)) return 1;
  tmhip_field *tmp = m->full_tmp;
  const double mu = ctx->mu;
  ctx->mu = -mu;
  const int e = tmhip_D_psi(ctx, l, k);
  ctx->mu = mu;
  if (e) return 1;
  for (int h = 0; h < 2; h++)
    if (tmhip_gamma5(ctx, tmp->half[h], l->half[h], ctx->Vh)) return 1;
  if (tmhip_D_psi(ctx, l, tmp)) return 1;
  for (int h = 0; h < 2; h++)
    if (tmhip_gamma5(ctx, l->half[h], l->half[h], ctx->Vh)) return 1;
  return 0;
}

// |f|^2 over N sites (FULL fields: both halves, even half first)
static int mms_norm(tmhip_ctx *ctx, tmhip_field *f, double *out) {
  if (f->kind == TMHIP_FIELD_EO) return tmhip_square_norm(ctx, f, ctx->Vh, 1, out);
  double a, b;
  if (tmhip_square_norm(ctx, f->half[0], ctx->Vh, 1, &a) || tmhip_square_norm(ctx, f->half[1], ctx->Vh, 1, &b)) return 1;
  *out = a + b;
  return 0;
}

static int mms_copy(tmhip_ctx *ctx, tmhip_field *dst, const tmhip_field *src) {
  const size_t bytes = (size_t)12 * ctx->ns * (dst->kind == TMHIP_FIELD_FULL ? 2 : 1) * sizeof(v2d);
  TMHIP_CHECK(hipMemcpyAsync(dst->d, src->d, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

// Which form an e/o solve takes on this context: the fused stencils need the shapes cg_her fuses (whole blocks of the launch)
static bool mms_fusable(const tmhip_ctx *ctx) { return ctx->opt_cg_fused_dot && ctx->Vh % tmhip_hop_block(ctx) == 0; }

static int mms_solve(tmhip_ctx *ctx, tmhip_field **P, tmhip_field *Q, const double *shifts, int nsh, int max_iter, double eps_sq,
                     int rel_prec, int op, int *iters, double *reached) {
  TmhipMms *m = (TmhipMms *)ctx->mms;
  const tmhip_op_row *row = tmhip_op_row_of(op);
  const int kind = row->kind;
  const bool full = kind == TMHIP_FIELD_FULL;
  for (int j = 0; j < 3; j++)
    if (!m->w[kind][j] && tmhip_field_alloc(ctx, kind, &m->w[kind][j])) return 1;
  for (; m->nps[kind] < nsh - 1; m->nps[kind]++)
    if (tmhip_field_alloc(ctx, kind, &m->ps[kind][m->nps[kind]])) return 1;
  tmhip_field *r = m->w[kind][0], *p = m->w[kind][1], *ap = m->w[kind][2];
  const bool clover = row->clover != TMHIP_SW_NONE;
  const double mu = ctx->mu, nrm = 1. / (1. + mu * mu);
  const size_t gs = ctx->gs;
  if (clover && fabs(mu) > 0 && ctx->sw_inv_sets < 2) TMHIP_FAIL("cg_mms_tm: Qsw_pm_psi with mu != 0 needs both sets of sw_inv (sw_invert with the current mu)");
  const int form = full ? 2 : (mms_fusable(ctx) ? 0 : 1);
  m->form = form;

  // start (cg_mms_tm.c:84-112): P_s = 0, ps_s = Q, r = p = Q, normsq = |Q|^2
  MshiftState h;
  memset(&h, 0, sizeof(h));
  double squarenorm;
  if (mms_norm(ctx, Q, &squarenorm)) return 1;
  for (int s = 0; s < nsh; s++)
    if (tmhip_field_zero(ctx, P[s])) return 1;
  h.sigma0 = shifts[0] * shifts[0];
  for (int s = 1; s < nsh; s++) {
    h.sigma[s] = shifts[s] * shifts[s] - h.sigma0;
    h.zita[s] = h.zitam1[s] = h.alphas[s] = 1.0;
    if (mms_copy(ctx, m->ps[kind][s - 1], Q)) return 1;
  }
  if (mms_copy(ctx, r, Q) || mms_copy(ctx, p, Q)) return 1;
  h.alpha0 = h.alphas[0] = 1.0; h.betas[0] = 0.0; h.normsq = squarenorm;
  h.target = rel_prec > 0 ? eps_sq * squarenorm : (rel_prec == 0 ? eps_sq : -1.0);   // :170-172: rel_prec < 0 runs to max_iter - 1
  h.eps_sq = eps_sq; h.active = h.pact = nsh; h.max_iter = max_iter; h.done_it = -1;
  v2d *tab[2 * MSHIFT_MAX_SHIFTS] = {};
  for (int s = 1; s < nsh; s++) { tab[2 * s] = P[s]->d; tab[2 * s + 1] = m->ps[kind][s - 1]->d; }
  TMHIP_CHECK(hipMemcpyAsync(m->tab, tab, sizeof(v2d *) * 2 * nsh, hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(m->st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));

  const int halves = full ? 2 : 1;
  const int nbl = (ctx->Vh + 255) / 256;
  const dim3 vg(nbl, halves);
  const int nvec = 4 * nbl * halves;
  if (nvec > m->max_partials) TMHIP_FAIL("cg_mms_tm: partials buffer too small");
  double *ppro = m->partials, *pr = m->partials + m->max_partials, *ppp = m->partials + 2 * m->max_partials, *psn = m->partials + 3 * m->max_partials;
  // |p|^2 of iteration 0 is |Q|^2: one value, then zeros (the same sum in the same order)
  TMHIP_CHECK(hipMemsetAsync(ppp, 0, (size_t)nvec * sizeof(double), ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(ppp, &squarenorm, sizeof(double), hipMemcpyHostToDevice, ctx->stream));

  const int batch = ctx->opt_cg_batch > 0 ? ctx->opt_cg_batch : 4;
  if (tmhip_poll_loop(ctx, max_iter, true, batch, 1.0e3 * (h.target > 0 ? h.target : eps_sq), &m->st->done, &m->st->err, 0, false, [&](int iteration) {
      const int check = nsh > 1 && iteration > 0 && iteration % 20 == 0;
      const int sn_next = nsh > 1 && (iteration + 1) % 20 == 0;
      int n1 = 0, n2 = nvec;
      const double *r_parts = form == 0 ? (const double *)ctx->partials : (const double *)pr;
      if (form == 0) {
        v2d *s0 = ctx->scratch[0]->d, *s1 = ctx->scratch[1]->d;
        const double *scal = &m->st->alpha0;   // {alpha0, sigma0}
        if (clover) {   // Qsw_pm_psi (clovertm_operators.c:233-245)
          const v2d *wim = ctx->sw_inv + (size_t)(fabs(mu) > 0 ? 1 : 0) * 72 * gs, *wip = ctx->sw_inv, *wo = ctx->sw + (size_t)54 * gs;
          if (tmhip_launch_hopping(ctx, TMHIP_EO, s1, p->d, nullptr, EPI_CLOVER_INV, 0, 0, HOP_COMM | HOP_FEED, wim)) return 1;
          if (tmhip_launch_hopping_dot(ctx, TMHIP_OE, s0, s1, p->d, nullptr, 0, -(mu + ctx->mu3), &n1, 1, nullptr, nullptr, wo, 3)) return 1;
          hipLaunchKernelGGL(mms_alpha_kernel, dim3(1), dim3(256), 0, ctx->stream, m->st, (const double *)ctx->partials, n1, (const double *)ppp, nvec);
          if (tmhip_launch_hopping(ctx, TMHIP_EO, s1, s0, nullptr, EPI_CLOVER_INV, 0, 0, HOP_COMM | HOP_CHAINED | HOP_FEED, wip)) return 1;
          if (tmhip_launch_hopping_dot(ctx, TMHIP_OE, nullptr, s1, s0, p->d, 0, +(mu + ctx->mu3), &n2, 3, r->d, scal, wo, 1)) return 1;
        } else {        // Qtm_pm_psi (tm_operators.c:338-345)
          if (tmhip_launch_hopping(ctx, TMHIP_EO, s1, p->d, nullptr, EPI_TM_TIMES, nrm, nrm * mu, HOP_COMM | HOP_FEED)) return 1;
          if (tmhip_launch_hopping_dot(ctx, TMHIP_OE, s0, s1, p->d, nullptr, 1., -mu, &n1, 1, nullptr, nullptr, nullptr, 3)) return 1;
          hipLaunchKernelGGL(mms_alpha_kernel, dim3(1), dim3(256), 0, ctx->stream, m->st, (const double *)ctx->partials, n1, (const double *)ppp, nvec);
          if (tmhip_launch_hopping(ctx, TMHIP_EO, s1, s0, nullptr, EPI_TM_TIMES, nrm, -nrm * mu, HOP_COMM | HOP_CHAINED | HOP_FEED)) return 1;
          if (tmhip_launch_hopping_dot(ctx, TMHIP_OE, nullptr, s1, s0, p->d, 1., mu, &n2, 3, r->d, scal, nullptr, 1)) return 1;
        }
      } else {
        if (tmhip_apply_op(ctx, op, ap, p)) return 1;
        hipLaunchKernelGGL(mms_dot_kernel, vg, dim3(256), 0, ctx->stream, (const MshiftState *)m->st, (const v2d *)p->d, (const v2d *)ap->d, ctx->ns, ctx->Vh, ppro);
        hipLaunchKernelGGL(mms_alpha_kernel, dim3(1), dim3(256), 0, ctx->stream, m->st, (const double *)ppro, nvec, (const double *)ppp, nvec);
        hipLaunchKernelGGL(mms_res_kernel, vg, dim3(256), 0, ctx->stream, (const MshiftState *)m->st, r->d, (const v2d *)ap->d, (const v2d *)p->d,
                           ctx->ns, ctx->Vh, pr);
      }
      hipLaunchKernelGGL(mms_beta_kernel, dim3(1), dim3(256), 0, ctx->stream, m->st, r_parts, n2, (const double *)psn, nvec, check, iteration);
      hipLaunchKernelGGL(mms_vec_kernel, vg, dim3(256), 0, ctx->stream, (const MshiftState *)m->st, (v2d *const *)m->tab, P[0]->d, p->d,
                         (const v2d *)r->d, ctx->ns, ctx->Vh, ppp, psn, sn_next, iteration);
      return 0;
    })) return 1;
  TMHIP_CHECK(hipMemcpyAsync(&h, m->st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (!h.done) TMHIP_FAIL("cg_mms_tm: the solve ended without its last iteration");
  ctx->mms_active_shifts = h.active;
  *iters = h.done_it == max_iter - 1 ? -1 : h.done_it + 1;   // cg_mms_tm.c:193-194
  if (reached) *reached = h.err;
  return 0;
}

extern "C" {

int tmhip_cg_mms_tm(tmhip_ctx *ctx, tmhip_field **P, tmhip_field *Q, const double *shifts, int nshifts, int max_iter, double eps_sq,
                    int rel_prec, int N, int op, int *iters, double *reached_prec) {
  if (nshifts < 1 || nshifts > MSHIFT_MAX_SHIFTS) TMHIP_FAIL("cg_mms_tm: nshifts = %d is outside [1, %d]", nshifts, MSHIFT_MAX_SHIFTS);
  if (!P || !Q || !shifts || !iters) TMHIP_FAIL("cg_mms_tm: null argument");
  if (tmhip_op_check(ctx, "cg_mms_tm", TMHIP_S_MMS, op, Q->kind)) return 1;
  const int kind = Q->kind;
  const bool full = kind == TMHIP_FIELD_FULL;
  if (N != (full ? ctx->V : ctx->Vh)) TMHIP_FAIL("cg_mms_tm: N = %d does not match the operator (%s needs %d)", N, full ? "Q_pm_psi" : "an e/o operator", full ? ctx->V : ctx->Vh);
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("cg_mms_tm: unsplit lattices only (nproc_t = %d%s)", ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  if (!ctx->gauge_set) TMHIP_FAIL("cg_mms_tm called before tmhip_set_gauge");
  if (max_iter < 1) TMHIP_FAIL("cg_mms_tm: max_iter < 1");
  if (Q->prec) TMHIP_FAIL("cg_mms_tm: Q must be an fp64 %s field", full ? "FULL" : "one-parity (EO)");
  for (int s = 0; s < nshifts; s++) {
    if (!P[s] || P[s]->kind != kind || P[s]->prec || P[s]->view) TMHIP_FAIL("cg_mms_tm: P[%d] must be an fp64 %s field", s, full ? "FULL" : "one-parity (EO)");
    if (P[s]->d == Q->d) TMHIP_FAIL("cg_mms_tm: a solution field is the source");
    for (int t = 0; t < s; t++)
      if (P[t]->d == P[s]->d) TMHIP_FAIL("cg_mms_tm: P[%d] and P[%d] are the same field", t, s);
  }
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (mms_prepare(ctx)) return 1;
  return mms_solve(ctx, P, Q, shifts, nshifts, max_iter, eps_sq, rel_prec, op, iters, reached_prec);
}

int tmhip_mms_active_shifts(tmhip_ctx *ctx) { return ctx->mms_active_shifts; }

int tmhip_mms_form(tmhip_ctx *ctx) { return ctx->mms ? ((TmhipMms *)ctx->mms)->form : -1; }

}  // extern "C"
