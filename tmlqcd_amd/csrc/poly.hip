// The polynomial monomial NDPOLY on the device (monomial/ndpoly_monomial.c, Ptilde_nd.c): fp64, Wilson twisted-mass doublet, unsplit
// lattices, the branch g_epsbar != 0 || phmc_exact_poly == 0 of all three bodies.
//
// The one new kernel is the four-term combination out = c1 A + c2 B + c3 C + c4 D (linalg/assign_mul_add_mul_add_mul_add_mul_r.c),
// added in the reference's order, element-wise on the SoA planes with 16 B per lane, BOTH flavours of a doublet in one launch
// (grid.z).  It is written with an output of its own so that Clenshaw's recursion (Ptilde_nd.c:141-189) needs no copy: the sv / aux /
// dd assigns of the reference become a rotation of three work doublets, a step is one Qsq plus one launch that writes the new d over
// the old dd.  out may be any of the inputs (no __restrict__ is claimed).
//
// Workspace, all owned by the context and kept until tmhip_destroy; the force gives back what a call with a smaller "poly_batch" or n no
// longer needs, and all of its work fields when one of its allocations fails:
//   Ptilde_ndpsi        3 doublets (d, dd, Qsq d)                                                     6 fields
//   ndpoly_derivative   the ascending chain chi[1 .. n-2] (chi[0] is pf itself)                       2 (n - 2) fields
//                       per group of G = "poly_batch" steps of the descending loop: G + 1 running chi_hi (the last of a group is
//                       the input of the next), G H_eo results of chi[j-1], G of chi_hi                6 G + 2 fields
//   ndpoly_heatbath     2 ping-pong doublets (+ Ptilde's)                                             4 fields
//   ndpoly_acc          the 8 chi doublets of :282-339 (+ Ptilde's)                                   16 fields
#include "tmhip_internal.h"

namespace polyhip {
struct Comb4 {
  v2d *out[2];
  const v2d *a[2], *b[2], *c[2], *d[2];
  double c1, c2, c3, c4;
};

__global__ __launch_bounds__(LA_BS, 8) void comb4_kernel(const Comb4 p, int ns, int N) {
  const int fl = blockIdx.z;
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *o = p.out[fl] + off;
  const v2d *a = p.a[fl] + off, *b = p.b[fl] + off, *c = p.c[fl] + off, *d = p.d[fl] + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      const v2d va = a[i], vb = b[i], vc = c[i], vd = d[i];
      o[i] = v2d{p.c1 * va.x + p.c2 * vb.x + p.c3 * vc.x + p.c4 * vd.x, p.c1 * va.y + p.c2 * vb.y + p.c3 * vc.y + p.c4 * vd.y};
    }
  }
}
}  // namespace polyhip
using namespace polyhip;

// ---------------------------------------------------------------- host side
#define POLY_MAX_GROUP 32
struct TmhipPoly {
  tmhip_field *cl[6];                          // Clenshaw: d, dd, Qsq d (s, c each)
  tmhip_field **chain; int nchain;             // chi[1 .. n-2] of the derivative, (up, dn) interleaved
  tmhip_field *hi[2 * (POLY_MAX_GROUP + 1)];   // running chi_hi of the descending loop
  tmhip_field *w[4 * POLY_MAX_GROUP];          // per step: H_eo chi[j-1] (s, c), H_eo chi_hi (s, c)
  tmhip_field *pp[4];                          // heatbath ping-pong
  tmhip_field *ac[16];                         // acceptance: chi[0 .. 7]
};

void tmhip_poly_destroy(tmhip_ctx *ctx) {
  TmhipPoly *p = (TmhipPoly *)ctx->poly;
  if (!p) return;
  for (tmhip_field *f : p->cl) tmhip_field_free(ctx, f);
  for (int k = 0; k < p->nchain; k++) tmhip_field_free(ctx, p->chain[k]);
  free(p->chain);
  for (tmhip_field *f : p->hi) tmhip_field_free(ctx, f);
  for (tmhip_field *f : p->w) tmhip_field_free(ctx, f);
  for (tmhip_field *f : p->pp) tmhip_field_free(ctx, f);
  for (tmhip_field *f : p->ac) tmhip_field_free(ctx, f);
  delete p;
  ctx->poly = nullptr;
}

static bool poly_eo(const tmhip_ctx *ctx, const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 0 && f->ns == ctx->ns; }

// everything that is refused is refused here, before any launch
static int poly_prepare(tmhip_ctx *ctx, const char *who, tmhip_field *a, tmhip_field *b, int op = TMHIP_ND_OP_QTM_PM) {
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: unsplit lattices only (nproc_t = %d%s)", who, ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  if (tmhip_nd_op_check(ctx, who, op)) return 1;
  if (!poly_eo(ctx, a) || !poly_eo(ctx, b)) TMHIP_FAIL("%s needs fp64 one-parity (EO) fields of this context's stride", who);
  if (a->d == b->d) TMHIP_FAIL("%s: the two flavours must be different fields", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->poly) ctx->poly = new TmhipPoly();
  return 0;
}
// Qtm_ndpsi, Qtm_dagger_ndpsi and Qtm_pm_ndpsi inside the bodies scale with the phmc_invmaxev of tmhip_set_nd, Q_tau1_sub_const_ndpsi with the
// argument (as in the reference, where ndpoly_set_global_parameter makes them one number): two different values would be an inconsistent monomial
static int poly_invmaxev(const tmhip_ctx *ctx, const char *who, double invmaxev) {
  if (invmaxev != ctx->invmaxev) TMHIP_FAIL("%s: invmaxev = %.17g is not the phmc_invmaxev of tmhip_set_nd (%.17g)", who, invmaxev, ctx->invmaxev);
  return 0;
}
static int poly_need(tmhip_ctx *ctx, tmhip_field **slot, int n) {
  for (int k = 0; k < n; k++) {
    if (slot[k]) continue;
    // "poly_fail_alloc" k (tests): the k-th allocation from here on fails, once, as an exhausted device would make it fail
    if (ctx->opt_poly_fail_alloc > 0 && --ctx->opt_poly_fail_alloc == 0) TMHIP_FAIL("ndpoly: field allocation failed (option poly_fail_alloc)");
    if (tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &slot[k])) return 1;
  }
  return 0;
}
static void poly_release(tmhip_ctx *ctx, tmhip_field **slot, int from, int to) {
  for (int k = from; k < to; k++) { tmhip_field_free(ctx, slot[k]); slot[k] = nullptr; }
}
static int poly_need_chain(tmhip_ctx *ctx, TmhipPoly *p, int n) {
  if (n > p->nchain) {
    tmhip_field **c = (tmhip_field **)realloc(p->chain, (size_t)n * sizeof(tmhip_field *));
    if (!c) TMHIP_FAIL("ndpoly_derivative: out of host memory");
    for (int k = p->nchain; k < n; k++) c[k] = nullptr;
    p->chain = c;
    // nchain counts the slots, filled or not: tmhip_field_free(nullptr) is a no-op
    p->nchain = n;
  }
  return poly_need(ctx, p->chain, n);
}

// out = c1 A + c2 B + c3 C + c4 D for nfl flavours (pointer pairs) over the Vh sites
static int poly_comb4(tmhip_ctx *ctx, int nfl, tmhip_field *const *out, tmhip_field *const *A, tmhip_field *const *B, tmhip_field *const *Cc,
                      tmhip_field *const *D, double c1, double c2, double c3, double c4) {
  Comb4 p;
  memset(&p, 0, sizeof(p));
  for (int f = 0; f < nfl; f++) { p.out[f] = out[f]->d; p.a[f] = A[f]->d; p.b[f] = B[f]->d; p.c[f] = Cc[f]->d; p.d[f] = D[f]->d; }
  p.c1 = c1; p.c2 = c2; p.c3 = c3; p.c4 = c4;
  dim3 grid = la_grid(ctx->Vh);
  grid.z = nfl;
  hipLaunchKernelGGL(comb4_kernel, grid, dim3(LA_BS), 0, ctx->stream, p, ctx->ns, ctx->Vh);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// Ptilde_nd.c:141-189 after the checks; R may be S, neither is one of the work fields
static int ptilde_body(tmhip_ctx *ctx, tmhip_field *R_s, tmhip_field *R_c, const double *dd, int n, tmhip_field *S_s, tmhip_field *S_c, double evmin,
                       double evmax, int op) {
  TmhipPoly *p = (TmhipPoly *)ctx->poly;
  if (poly_need(ctx, p->cl, 6)) return 1;
  const double fact1 = 4 / (evmax - evmin), fact2 = -2 * (evmax + evmin) / (evmax - evmin);   // :141-142
  tmhip_field *d[2] = {p->cl[0], p->cl[1]}, *e[2] = {p->cl[2], p->cl[3]}, *q[2] = {p->cl[4], p->cl[5]};
  tmhip_field *R[2] = {R_s, R_c}, *S[2] = {S_s, S_c};
  for (int f = 0; f < 2; f++)
    if (tmhip_field_zero(ctx, d[f]) || tmhip_field_zero(ctx, e[f])) return 1;   // :144-147
  for (int j = n - 1; j >= 1; j--) {                                          // :154-175
    if (tmhip_apply_nd_op(ctx, op, q[0], q[1], d[0], d[1])) return 1;
    if (poly_comb4(ctx, 2, e, d, q, e, S, fact2, fact1, -1.0, dd[j])) return 1;   // the new d over the old dd
    for (int f = 0; f < 2; f++) { tmhip_field *t = d[f]; d[f] = e[f]; e[f] = t; }
  }
  if (tmhip_apply_nd_op(ctx, op, q[0], q[1], d[0], d[1])) return 1;            // :180
  return poly_comb4(ctx, 2, R, q, d, e, S, fact1 / 2, fact2 / 2, -1.0, dd[0] / 2);   // :182-189
}

static int poly_norm2(tmhip_ctx *ctx, tmhip_field *a, tmhip_field *b, double *out) {
  double ea, eb;
  if (tmhip_square_norm(ctx, a, ctx->Vh, 1, &ea) || tmhip_square_norm(ctx, b, ctx->Vh, 1, &eb)) return 1;
  *out = ea + eb;
  return 0;
}

extern "C" {

int tmhip_assign_mul_add_mul_add_mul_add_mul_r(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, tmhip_field *V, double c1, double c2,
                                               double c3, double c4) {
  if (!poly_eo(ctx, R) || !poly_eo(ctx, S) || !poly_eo(ctx, U) || !poly_eo(ctx, V))
    TMHIP_FAIL("assign_mul_add_mul_add_mul_add_mul_r needs fp64 one-parity (EO) fields of this context's stride");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  return poly_comb4(ctx, 1, &R, &R, &S, &U, &V, c1, c2, c3, c4);
}

int tmhip_comb4_ndpsi(tmhip_ctx *ctx, tmhip_field *out_s, tmhip_field *out_c, tmhip_field *A_s, tmhip_field *A_c, tmhip_field *B_s, tmhip_field *B_c,
                      tmhip_field *C_s, tmhip_field *C_c, tmhip_field *D_s, tmhip_field *D_c, double c1, double c2, double c3, double c4) {
  tmhip_field *o[2] = {out_s, out_c}, *A[2] = {A_s, A_c}, *B[2] = {B_s, B_c}, *Cc[2] = {C_s, C_c}, *D[2] = {D_s, D_c};
  for (int f = 0; f < 2; f++)
    if (!poly_eo(ctx, o[f]) || !poly_eo(ctx, A[f]) || !poly_eo(ctx, B[f]) || !poly_eo(ctx, Cc[f]) || !poly_eo(ctx, D[f]))
      TMHIP_FAIL("comb4_ndpsi needs fp64 one-parity (EO) fields of this context's stride");
  if (out_s->d == out_c->d) TMHIP_FAIL("comb4_ndpsi: the two output flavours must be different fields");
  for (int f = 0; f < 2; f++)   // the other flavour is read by other blocks of the same launch
    if (o[f]->d == A[1 - f]->d || o[f]->d == B[1 - f]->d || o[f]->d == Cc[1 - f]->d || o[f]->d == D[1 - f]->d)
      TMHIP_FAIL("comb4_ndpsi: an output may be an input of its own flavour only");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  return poly_comb4(ctx, 2, o, A, B, Cc, D, c1, c2, c3, c4);
}

int tmhip_Ptilde_ndpsi(tmhip_ctx *ctx, tmhip_field *R_s, tmhip_field *R_c, const double *coefs, int n, tmhip_field *S_s, tmhip_field *S_c, double evmin,
                       double evmax, int op) {
  if (n < 1 || !coefs) TMHIP_FAIL("Ptilde_ndpsi: n = %d coefficients (needs n >= 1 and a coefficient array)", n);
  if (!(evmax > evmin)) TMHIP_FAIL("Ptilde_ndpsi: the interval [%g, %g] is empty", evmin, evmax);
  if (poly_prepare(ctx, "Ptilde_ndpsi", R_s, R_c, op) || poly_prepare(ctx, "Ptilde_ndpsi", S_s, S_c, op)) return 1;
  if (R_s->d == S_c->d || R_c->d == S_s->d) TMHIP_FAIL("Ptilde_ndpsi: R may be S flavour by flavour only (R_s = S_s, R_c = S_c)");
  return ptilde_body(ctx, R_s, R_c, coefs, n, S_s, S_c, evmin, evmax, op);
}

int tmhip_ndpoly_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev) {
  if (n < 3 || !roots) TMHIP_FAIL("ndpoly_derivative: n = %d (MDPolyDegree, needs n >= 3 and 2n - 2 roots)", n);
  if (poly_prepare(ctx, "ndpoly_derivative", pf_up, pf_dn) || poly_invmaxev(ctx, "ndpoly_derivative", invmaxev)) return 1;
  TmhipPoly *p = (TmhipPoly *)ctx->poly;
  const int nsteps = n - 1;
  int G = ctx->opt_poly_batch < 1 ? 1 : (ctx->opt_poly_batch > POLY_MAX_GROUP ? POLY_MAX_GROUP : ctx->opt_poly_batch);
  if (G > nsteps) G = nsteps;
  // what a larger group or a longer chain of an earlier call holds beyond this call's need goes back first
  poly_release(ctx, p->hi, 2 * (G + 1), 2 * (POLY_MAX_GROUP + 1));
  poly_release(ctx, p->w, 4 * G, 4 * POLY_MAX_GROUP);
  if (p->nchain > 2 * (n - 2)) poly_release(ctx, p->chain, 2 * (n - 2), p->nchain);
  // every allocation before the first launch: a failure leaves the accumulator as it was, and the force keeps none of its work fields
  if (poly_need_chain(ctx, p, 2 * (n - 2)) || poly_need(ctx, p->hi, 2 * (G + 1)) || poly_need(ctx, p->w, 4 * G) ||
      (!ctx->deriv && tmhip_derivative_zero(ctx))) {
    poly_release(ctx, p->chain, 0, p->nchain);
    poly_release(ctx, p->hi, 0, 2 * (POLY_MAX_GROUP + 1));
    poly_release(ctx, p->w, 0, 4 * POLY_MAX_GROUP);
    return 1;
  }
  const double ff = -Cpol * invmaxev;   // mnl->forcefactor (:69)
  // chi[0] = pf (:79-80, read only), chi[k] = Q_tau1_sub_const(chi[k-1], roots[k-1]) for k = 1 .. n-2 (:82-86)
  auto chi = [&](int k, int f) { return k == 0 ? (f ? pf_dn : pf_up) : p->chain[2 * (k - 1) + f]; };
  for (int k = 1; k <= n - 2; k++)
    if (tmhip_Q_tau1_sub_const_ndpsi(ctx, chi(k, 0), chi(k, 1), chi(k - 1, 0), chi(k - 1, 1), roots[2 * (k - 1)], roots[2 * (k - 1) + 1], Cpol, invmaxev)) return 1;
  // the descending loop (:94-117): step s = 0 .. n-2 is j = n-1-s; its chi_hi lives in slot (s + 1) mod (G + 1), its input in slot s mod (G + 1)
  tmhip_field *in[2] = {chi(n - 2, 0), chi(n - 2, 1)};   // :91-92
  for (int s0 = 0; s0 < nsteps; s0 += G) {
    const int g = nsteps - s0 < G ? nsteps - s0 : G;
    tmhip_field *l0[2 * POLY_MAX_GROUP], *k0[2 * POLY_MAX_GROUP], *l1[2 * POLY_MAX_GROUP], *k1[2 * POLY_MAX_GROUP];
    double fac[2 * POLY_MAX_GROUP];
    for (int q = 0; q < g; q++) {
      const int s = s0 + q, j = n - 1 - s;
      tmhip_field **hi = p->hi + 2 * ((s + 1) % (G + 1)), **w = p->w + 4 * q;
      const double *z = roots + 2 * (2 * n - 3 - j);
      if (tmhip_Q_tau1_sub_const_ndpsi(ctx, hi[0], hi[1], in[0], in[1], z[0], z[1], Cpol, invmaxev)) return 1;   // :98-100
      if (tmhip_H_eo_tm_ndpsi(ctx, w[0], w[1], chi(j - 1, 0), chi(j - 1, 1), TMHIP_EO)) return 1;                  // :103-104
      if (G == 1) {   // the reference's call order on the single-pair kernel
        if (tmhip_deriv_Sb(ctx, TMHIP_EO, w[0], hi[0], ff) || tmhip_deriv_Sb(ctx, TMHIP_EO, w[1], hi[1], ff)) return 1;     // :107-108
        if (tmhip_H_eo_tm_ndpsi(ctx, w[2], w[3], hi[0], hi[1], TMHIP_EO)) return 1;                                        // :111-112
        if (tmhip_deriv_Sb(ctx, TMHIP_OE, chi(j - 1, 0), w[2], ff) || tmhip_deriv_Sb(ctx, TMHIP_OE, chi(j - 1, 1), w[3], ff)) return 1;   // :115-116
      } else {
        if (tmhip_H_eo_tm_ndpsi(ctx, w[2], w[3], hi[0], hi[1], TMHIP_EO)) return 1;
        l0[2 * q] = w[0]; k0[2 * q] = hi[0]; l0[2 * q + 1] = w[1]; k0[2 * q + 1] = hi[1];
        l1[2 * q] = chi(j - 1, 0); k1[2 * q] = w[2]; l1[2 * q + 1] = chi(j - 1, 1); k1[2 * q + 1] = w[3];
        fac[2 * q] = fac[2 * q + 1] = ff;
      }
      in[0] = hi[0]; in[1] = hi[1];
    }
    if (G > 1 && (tmhip_deriv_Sb_batch(ctx, TMHIP_EO, 2 * g, l0, k0, fac) || tmhip_deriv_Sb_batch(ctx, TMHIP_OE, 2 * g, l1, k1, fac))) return 1;
  }
  return 0;
}

int tmhip_ndpoly_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev,
                          const double *ptilde_coefs, int ptilde_n, double evmin, double evmax, double *energy0) {
  if (n < 2 || !roots || !ptilde_coefs || ptilde_n < 1 || !energy0) TMHIP_FAIL("ndpoly_heatbath: n = %d, ptilde_n = %d or a null argument", n, ptilde_n);
  if (!(evmax > evmin)) TMHIP_FAIL("ndpoly_heatbath: the interval [%g, %g] is empty", evmin, evmax);
  if (poly_prepare(ctx, "ndpoly_heatbath", pf_up, pf_dn) || poly_invmaxev(ctx, "ndpoly_heatbath", invmaxev)) return 1;
  TmhipPoly *p = (TmhipPoly *)ctx->poly;
  if (poly_need(ctx, p->pp, 4) || poly_need(ctx, p->cl, 6)) return 1;
  if (poly_norm2(ctx, pf_up, pf_dn, energy0)) return 1;                              // :181,185
  tmhip_field *a[2] = {p->pp[0], p->pp[1]}, *b[2] = {p->pp[2], p->pp[3]};
  if (tmhip_Qtm_ndpsi(ctx, a[0], a[1], pf_up, pf_dn)) return 1;                      // :196-197
  for (int j = 1; j < n; j++) {                                                      // :199-206, ping-pong for the two assigns
    const double *z = roots + 2 * (n - 2 + j);
    if (tmhip_Q_tau1_sub_const_ndpsi(ctx, b[0], b[1], a[0], a[1], z[0], z[1], Cpol, invmaxev)) return 1;
    for (int f = 0; f < 2; f++) { tmhip_field *t = a[f]; a[f] = b[f]; b[f] = t; }
  }
  return ptilde_body(ctx, pf_up, pf_dn, ptilde_coefs, ptilde_n, a[0], a[1], evmin, evmax, TMHIP_ND_OP_QTM_PM);   // :207-208, 255-256
}

int tmhip_ndpoly_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *roots, int n, double Cpol, double invmaxev,
                     const double *md_coefs, const double *ptilde_coefs, int ptilde_n, double evmin, double evmax, double precision_hfinal,
                     double *energy1, int *corrections, double *ener) {
  if (n < 2 || !roots || !md_coefs || !ptilde_coefs || ptilde_n < 1 || !energy1 || !corrections)
    TMHIP_FAIL("ndpoly_acc: n = %d, ptilde_n = %d or a null argument", n, ptilde_n);
  if (!(evmax > evmin)) TMHIP_FAIL("ndpoly_acc: the interval [%g, %g] is empty", evmin, evmax);
  if (poly_prepare(ctx, "ndpoly_acc", pf_up, pf_dn) || poly_invmaxev(ctx, "ndpoly_acc", invmaxev)) return 1;
  TmhipPoly *p = (TmhipPoly *)ctx->poly;
  if (poly_need(ctx, p->ac, 16) || poly_need(ctx, p->cl, 6)) return 1;
  double Ener[8], factor[8];
  factor[0] = 1.0; Ener[0] = 0;
  for (int j = 1; j < 8; j++) { factor[j] = j * factor[j - 1]; Ener[j] = 0; }
  tmhip_field *chi[8][2];
  for (int j = 0; j < 8; j++) { chi[j][0] = p->ac[2 * j]; chi[j][1] = p->ac[2 * j + 1]; }
  // the chain (:287-298): chi[0] and chi[1] swap roles instead of the copy of :301-304
  tmhip_field *in[2] = {pf_up, pf_dn};
  for (int j = 1; j <= n - 1; j++) {
    tmhip_field **out = (in[0] == chi[0][0]) ? chi[1] : chi[0];
    if (tmhip_Q_tau1_sub_const_ndpsi(ctx, out[0], out[1], in[0], in[1], roots[2 * (j - 1)], roots[2 * (j - 1) + 1], Cpol, invmaxev)) return 1;
    in[0] = out[0]; in[1] = out[1];
  }
  if (in[0] == chi[1][0]) for (int f = 0; f < 2; f++) { tmhip_field *t = chi[0][f]; chi[0][f] = chi[1][f]; chi[1][f] = t; }
  if (poly_norm2(ctx, chi[0][0], chi[0][1], &Ener[0])) return 1;   // :306-310
  int j, ij = 0;
  for (j = 1; j < 8; j++) {
    tmhip_field **c1 = chi[j], **c0 = chi[j - 1];
    if (j % 2) {   // chi[j] = (Qdag P Ptilde) chi[j-1]   (:319-329)
      if (ptilde_body(ctx, c1[0], c1[1], ptilde_coefs, ptilde_n, c0[0], c0[1], evmin, evmax, TMHIP_ND_OP_QTM_PM)) return 1;
      if (ptilde_body(ctx, c0[0], c0[1], md_coefs, n, c1[0], c1[1], evmin, evmax, TMHIP_ND_OP_QTM_PM)) return 1;
      if (tmhip_Qtm_dagger_ndpsi(ctx, c1[0], c1[1], c0[0], c0[1])) return 1;
    } else {       // chi[j] = (Ptilde P Q) chi[j-1]      (:330-339)
      if (tmhip_Qtm_ndpsi(ctx, c1[0], c1[1], c0[0], c0[1])) return 1;
      if (ptilde_body(ctx, c0[0], c0[1], md_coefs, n, c1[0], c1[1], evmin, evmax, TMHIP_ND_OP_QTM_PM)) return 1;
      if (ptilde_body(ctx, c1[0], c1[1], ptilde_coefs, ptilde_n, c0[0], c0[1], evmin, evmax, TMHIP_ND_OP_QTM_PM)) return 1;
    }
    Ener[j] = Ener[j - 1] + Ener[0];   // :341-357
    double sgn = -1.0, temp;
    for (ij = 1; ij < j; ij++) {
      const double fact = factor[j] / (factor[ij] * factor[j - ij]);
      Ener[j] += sgn * fact * Ener[ij];
      sgn = -sgn;
    }
    if (poly_norm2(ctx, c1[0], c1[1], &temp)) return 1;
    Ener[j] += sgn * temp;
    if (fabs(Ener[j] - Ener[j - 1]) < precision_hfinal) break;   // :359-366
  }
  *energy1 = Ener[ij];                   // :368, "quite sticky": ij is where the inner loop stopped
  *corrections = j < 8 ? j : 7;
  if (ener) memcpy(ener, Ener, sizeof(Ener));
  return 0;
}

}  // extern "C"
