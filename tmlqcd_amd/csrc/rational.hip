// Rational monomials on the device: rat (monomial/rat_monomial.c, types RAT and CLOVERRAT) and ndrat (monomial/ndrat_monomial.c, types
// NDRAT and NDCLOVERRAT), fp64, unsplit lattices; at the end of the file the correction monomials ratcor / ndratcor on top of them.
//
// The hot path is the hopping force.  ndrat_derivative calls deriv_Sb four times per shift (ndrat_monomial.c:140-160), rat_derivative
// twice (rat_monomial.c:124-131); every call reads the same four links per site and does a read-modify-write of the same 32
// derivative reals.  deriv_Sb_batch_kernel sums n (l, k, factor) pairs in ONE launch with the ownership of deriv_Sb_kernel
// (force.hip: one thread per site of either parity owns its four forward links, no atomics): per link it accumulates
//   T = sum_j 2 factor_j (v_j (x) u_j^dagger + z_j (x) w_j^dagger)          (3x3 complex; the coefficient is folded into v_j, z_j)
// over the pairs, then forms ka_mu U_mu T once and projects it with the su3adj.h rule into the derivative field: links are read
// once and the derivative is written once per launch, whatever n is.
//
// The directions are the outer loop: one T is live and the own-site spinor of a pair is read again per direction (from cache):
// 164 VGPRs, three waves per SIMD, no scratch.  The other order (pairs outermost, four T live, every spinor read once) needs
// 144 registers for the accumulators alone and spills at the two waves per SIMD the kernel is held to (tools/check_resources.py).
//
// The monomial bodies below are the reference's loops with the solutions kept in HBM: force (given the solutions), derivative
// (solve + force), heatbath and acceptance energy.
#include "tmhip_internal.h"
#include "mshift.h"

namespace rathip {

struct BatchArgs {
  const v2d *l[RAT_MAX_PAIRS], *k[RAT_MAX_PAIRS];
  double fac[RAT_MAX_PAIRS];   // 2 * factor_j
  const v2d *g;                // gauge [2][8][9][gs]
  double *deriv;               // [2][4][8][Vh]
  int n, ns, gs, Vh, T, LX, LY, LZ, ieo;
  double ka[4][2];
};

__device__ __forceinline__ v2d b_cmul(v2d a, v2d b) { return v2d{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ v2d b_cmulc(v2d a, v2d b) { return v2d{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }   // a conj(b)
__device__ __forceinline__ v2d b_itimes(v2d a) { return v2d{-a.y, a.x}; }

// (1 +- gamma_mu) of a 4-spinor s[spin][colour] as two 3-vectors; the lines of f_project (force.hip), MU a compile-time constant
template <int MU>
__device__ __forceinline__ void b_project(const v2d (&s)[4][3], bool plus, v2d (&a)[3], v2d (&b)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (MU == 0) { a[c] = plus ? s[0][c] + s[2][c] : s[0][c] - s[2][c]; b[c] = plus ? s[1][c] + s[3][c] : s[1][c] - s[3][c]; }
    if (MU == 1) { a[c] = plus ? s[0][c] + b_itimes(s[3][c]) : s[0][c] - b_itimes(s[3][c]);
                   b[c] = plus ? s[1][c] + b_itimes(s[2][c]) : s[1][c] - b_itimes(s[2][c]); }
    if (MU == 2) { a[c] = plus ? s[0][c] + s[3][c] : s[0][c] - s[3][c]; b[c] = plus ? s[1][c] - s[2][c] : s[1][c] + s[2][c]; }
    if (MU == 3) { a[c] = plus ? s[0][c] + b_itimes(s[2][c]) : s[0][c] - b_itimes(s[2][c]);
                   b[c] = plus ? s[1][c] - b_itimes(s[3][c]) : s[1][c] + b_itimes(s[3][c]); }
  }
}

// the fields are only read, and one field may serve several pairs on either side: no __restrict__ between them is claimed
__device__ __forceinline__ void b_load(const v2d *f, int ns, int idx, bool g5, v2d (&s)[4][3]) {
#pragma unroll
  for (int sp = 0; sp < 4; sp++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      v2d v = f[(size_t)(3 * sp + c) * ns + idx];
      if (g5 && sp >= 2) v = v2d{-v.x, -v.y};
      s[sp][c] = v;
    }
}

// T += fac (v (x) u^dagger + z (x) w^dagger) for direction MU of one pair; own / nb: the site's and the +mu neighbour's spinor.
// "+" sites (parity == ieo) carry g5 l, the neighbour k: (v, z) = projections of k, (u, w) = of g5 l.  "-" sites the other way round.
template <int MU>
__device__ __forceinline__ void b_accum(v2d (&t)[9], const v2d (&own)[4][3], const v2d (&nb)[4][3], bool plus, double fac) {
  v2d oa[3], ob[3], na[3], nb2[3];
  b_project<MU>(own, plus, oa, ob);
  b_project<MU>(nb, plus, na, nb2);
  // deriv_Sb_kernel: plus: (v, z) = (psia, psib) = nb, (u, w) = (phia, phib) = own;  minus: (v, z) = (phia, phib) = nb, (u, w) = (psia, psib) = own
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const v2d v = fac * na[r], z = fac * nb2[r];
#pragma unroll
    for (int c = 0; c < 3; c++) t[3 * r + c] += b_cmulc(v, oa[c]) + b_cmulc(z, ob[c]);
  }
}

// df(y, mu) += trlambda(ka_mu U_mu(y) T)   (su3adj.h:164-172)
__device__ __forceinline__ void b_finish(const v2d (&t)[9], const v2d *gp, size_t gs, int mu, v2d ka, double *d, size_t st) {
  v2d U[9];
#pragma unroll
  for (int e = 0; e < 9; e++) U[e] = gp[(size_t)((2 * mu) * 9 + e) * gs];
  v2d m[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++)
      m[r][c] = b_cmul(ka, b_cmul(U[3 * r], t[c]) + b_cmul(U[3 * r + 1], t[3 + c]) + b_cmul(U[3 * r + 2], t[6 + c]));
  d[0 * st] += (-m[1][0].y - m[0][1].y);
  d[1 * st] += (+m[1][0].x - m[0][1].x);
  d[2 * st] += (-m[0][0].y + m[1][1].y);
  d[3 * st] += (-m[2][0].y - m[0][2].y);
  d[4 * st] += (+m[2][0].x - m[0][2].x);
  d[5 * st] += (-m[2][1].y - m[1][2].y);
  d[6 * st] += (+m[2][1].x - m[1][2].x);
  d[7 * st] += ((-m[0][0].y - m[1][1].y + 2.0 * m[2][2].y) * 0.577350269189625);
}

__global__ __launch_bounds__(128, 2) void deriv_Sb_batch_kernel(const BatchArgs a) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= a.Vh) return;
  const int par = blockIdx.y;
  const bool plus = par == a.ieo;         // this site carries the left vectors l_j
  const int LZh = a.LZ / 2;
  const int kz = i % LZh;
  int r = i / LZh;
  const int y = r % a.LY;
  r /= a.LY;
  const int x = r % a.LX, t = r / a.LX;
  const int o = (t + x + y + par) & 1;
  const int z = 2 * kz + o;
  const int row = (t * a.LX + x) * a.LY + y;   // lexic = row * LZ + z
  int up[4];
  up[0] = ((((t + 1) % a.T) * a.LX + x) * a.LY + y) * LZh + kz;
  up[1] = ((t * a.LX + (x + 1) % a.LX) * a.LY + y) * LZh + kz;
  up[2] = ((t * a.LX + x) * a.LY + (y + 1) % a.LY) * LZh + kz;
  up[3] = (row * a.LZ + (z + 1) % a.LZ) >> 1;
  const v2d *gp = a.g + (size_t)par * 72 * a.gs + i;
  double *dp = a.deriv + (size_t)par * 32 * a.Vh + i;
  const size_t st = a.Vh;
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {
    v2d t1[9];
#pragma unroll
    for (int e = 0; e < 9; e++) t1[e] = v2d{0.0, 0.0};
    for (int j = 0; j < a.n; j++) {
      const v2d *fo = plus ? a.l[j] : a.k[j], *fn = plus ? a.k[j] : a.l[j];
      v2d own[4][3], nb[4][3];
      b_load(fo, a.ns, i, plus, own);
      b_load(fn, a.ns, up[mu], !plus, nb);
      if (mu == 0) b_accum<0>(t1, own, nb, plus, a.fac[j]);
      if (mu == 1) b_accum<1>(t1, own, nb, plus, a.fac[j]);
      if (mu == 2) b_accum<2>(t1, own, nb, plus, a.fac[j]);
      if (mu == 3) b_accum<3>(t1, own, nb, plus, a.fac[j]);
    }
    b_finish(t1, gp, a.gs, mu, v2d{a.ka[mu][0], a.ka[mu][1]}, dp + (size_t)mu * 8 * st, st);
  }
}
}  // namespace rathip
using namespace rathip;

// ---------------------------------------------------------------- host side
struct TmhipRat {
  tmhip_field *chi_up[MSHIFT_MAX_SHIFTS], *chi_dn[MSHIFT_MAX_SHIFTS];   // solutions of the drivers (allocated as needed)
  tmhip_field *w[6 * MSHIFT_MAX_SHIFTS];                               // work fields of the force groups, heatbath and acceptance
};

void tmhip_rat_destroy(tmhip_ctx *ctx) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (!r) return;
  for (int k = 0; k < MSHIFT_MAX_SHIFTS; k++) { tmhip_field_free(ctx, r->chi_up[k]); tmhip_field_free(ctx, r->chi_dn[k]); }
  for (int k = 0; k < 6 * MSHIFT_MAX_SHIFTS; k++) tmhip_field_free(ctx, r->w[k]);
  delete r;
  ctx->rat = nullptr;
}

static int rat_prepare(tmhip_ctx *ctx, const char *who, int np) {
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: unsplit lattices only (nproc_t = %d%s)", who, ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  if (np < 1 || np > MSHIFT_MAX_SHIFTS) TMHIP_FAIL("%s: np = %d is outside [1, %d]", who, np, MSHIFT_MAX_SHIFTS);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->rat) ctx->rat = new TmhipRat();
  return 0;
}
static int rat_need(tmhip_ctx *ctx, tmhip_field **slot, int n) {
  for (int k = 0; k < n; k++)
    if (!slot[k] && tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &slot[k])) return 1;
  return 0;
}
static bool rat_eo(const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 0; }
static int rat_group(const tmhip_ctx *ctx) { return ctx->opt_rat_batch < 1 ? 1 : (ctx->opt_rat_batch > MSHIFT_MAX_SHIFTS ? MSHIFT_MAX_SHIFTS : ctx->opt_rat_batch); }

// rat runs at twisted mass 0 (rat_monomial.c:62,156,222): the context's mu is put back on every path out
struct RatMuZero {
  tmhip_ctx *ctx; double mu, mu3;
  // sw: the clover operators twist their odd-odd term with mu + mu3 (rat_monomial.c:63,157,223 zero g_mu3 as well)
  explicit RatMuZero(tmhip_ctx *c, bool sw = false) : ctx(c), mu(c->mu), mu3(c->mu3) { c->mu = 0.0; if (sw) c->mu3 = 0.0; }
  ~RatMuZero() { ctx->mu = mu; ctx->mu3 = mu3; }
};

// sw: type NDCLOVERRAT -- the clover operators, and the four sw_spinor_eo of ndrat_monomial.c:164-175 per shift: summed per group by one
// sw_spinor_eo_batch launch per parity (clover.hip), or with "rat_batch" 1 by the per-call kernel in the reference's order
static int ndrat_force_body(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev,
                            bool sw = false) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  const int G = rat_group(ctx);
  if (rat_need(ctx, r->w, 6 * (G < np ? G : np))) return 1;
  for (int hi = np - 1; hi >= 0; hi -= G) {   // the reference walks j downwards (ndrat_monomial.c:114)
    const int lo = hi - G + 1 > 0 ? hi - G + 1 : 0, g = hi - lo + 1;
    tmhip_field *l0[RAT_MAX_PAIRS], *k0[RAT_MAX_PAIRS], *l1[RAT_MAX_PAIRS], *k1[RAT_MAX_PAIRS];
    double f[RAT_MAX_PAIRS];
    for (int q = 0; q < g; q++) {
      const int j = hi - q;
      tmhip_field **w = r->w + 6 * q;
      // Y_j,o = (Q_h tau^1 + i mu_j) X_j,o (:130-132), X_j,e (:136-137), Y_j,e (:152-153)
      if (sw) {   // :118-125, :147-148
        if (tmhip_Qsw_tau1_sub_const_ndpsi(ctx, w[0], w[1], chi_up[j], chi_dn[j], 0.0, -mu[j], 1.0, invmaxev)) return 1;
        if (tmhip_H_eo_sw_ndpsi(ctx, w[2], w[3], chi_up[j], chi_dn[j])) return 1;
        if (tmhip_H_eo_sw_ndpsi(ctx, w[4], w[5], w[0], w[1])) return 1;
      } else {
        if (tmhip_Q_tau1_sub_const_ndpsi(ctx, w[0], w[1], chi_up[j], chi_dn[j], 0.0, -mu[j], 1.0, invmaxev)) return 1;
        if (tmhip_H_eo_tm_ndpsi(ctx, w[2], w[3], chi_up[j], chi_dn[j], TMHIP_EO)) return 1;
        if (tmhip_H_eo_tm_ndpsi(ctx, w[4], w[5], w[0], w[1], TMHIP_EO)) return 1;
      }
      f[2 * q] = f[2 * q + 1] = rmu[j] * invmaxev;                                      // forcefactor = EVMaxInv (:94)
      l0[2 * q] = w[2]; k0[2 * q] = w[0]; l0[2 * q + 1] = w[3]; k0[2 * q + 1] = w[1];   // deriv_Sb(EO, ..) (:140-143)
      l1[2 * q] = chi_up[j]; k1[2 * q] = w[4]; l1[2 * q + 1] = chi_dn[j]; k1[2 * q + 1] = w[5];   // deriv_Sb(OE, ..) (:157-160)
    }
    if (tmhip_deriv_Sb_batch(ctx, TMHIP_EO, 2 * g, l0, k0, f) || tmhip_deriv_Sb_batch(ctx, TMHIP_OE, 2 * g, l1, k1, f)) return 1;
    for (int q = 0; sw && G == 1 && q < g; q++) {   // :164-175: EE (w5, w2), OO (chi_up, w1), EE (w4, w3), OO (chi_dn, w0)
      const int j = hi - q;
      tmhip_field **w = r->w + 6 * q;
      if (tmhip_sw_spinor_eo(ctx, 0, w[5], w[2], f[2 * q]) || tmhip_sw_spinor_eo(ctx, 1, chi_up[j], w[1], f[2 * q])) return 1;
      if (tmhip_sw_spinor_eo(ctx, 0, w[4], w[3], f[2 * q]) || tmhip_sw_spinor_eo(ctx, 1, chi_dn[j], w[0], f[2 * q])) return 1;
    }
    if (sw && G > 1) {   // the same 4 g pairs: l0 / k0 / l1 / k1 are free again
      for (int q = 0; q < g; q++) {
        const int j = hi - q;
        tmhip_field **w = r->w + 6 * q;
        l0[2 * q] = w[5]; k0[2 * q] = w[2]; l0[2 * q + 1] = w[4]; k0[2 * q + 1] = w[3];
        l1[2 * q] = chi_up[j]; k1[2 * q] = w[1]; l1[2 * q + 1] = chi_dn[j]; k1[2 * q + 1] = w[0];
      }
      if (tmhip_sw_spinor_eo_batch(ctx, 0, 2 * g, l0, k0, f) || tmhip_sw_spinor_eo_batch(ctx, 1, 2 * g, l1, k1, f)) return 1;
    }
  }
  return 0;
}

// the clover monomial: refused before any launch unless the clover term and its doublet inverse are those of the current links
static int ndcloverrat_prepare(tmhip_ctx *ctx, const char *who, int np) {
  if (rat_prepare(ctx, who, np)) return 1;
  if (tmhip_ndsw_ready(ctx, who, true)) return 1;
  // the force ends in sw_all on the links tmhip_sw_term kept: a clover term uploaded with tmhip_set_clover has none
  if (!ctx->gauge_raw_valid) TMHIP_FAIL("%s: no lexicographic links on the device: the clover term must come from tmhip_sw_term, not tmhip_set_clover", who);
  return 0;
}
// ndrat_monomial.c:80-86 before the loop, :179-184 after it
static int ndcloverrat_force_all(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev,
                                 double kappa, double c_sw, int trlog) {
  if (tmhip_swpm_zero(ctx)) return 1;
  if (ndrat_force_body(ctx, chi_up, chi_dn, mu, rmu, np, invmaxev, true)) return 1;
  if (trlog && tmhip_sw_deriv_nd(ctx, 0)) return 1;
  return tmhip_sw_all(ctx, nullptr, kappa, c_sw);
}

// sw: type CLOVERRAT (rat_monomial.c:97-118) -- the clover operators at twisted mass 0, and the two sw_spinor_eo per shift
static int rat_force_body(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np, bool sw = false) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  const int G = rat_group(ctx);
  if (rat_need(ctx, r->w, 3 * (G < np ? G : np))) return 1;
  for (int hi = np - 1; hi >= 0; hi -= G) {   // rat_monomial.c:95
    const int lo = hi - G + 1 > 0 ? hi - G + 1 : 0, g = hi - lo + 1;
    tmhip_field *l0[RAT_MAX_PAIRS], *k0[RAT_MAX_PAIRS], *l1[RAT_MAX_PAIRS], *k1[RAT_MAX_PAIRS];
    double f[RAT_MAX_PAIRS];
    for (int q = 0; q < g; q++) {
      const int j = hi - q;
      tmhip_field *w0 = r->w[3 * q], *w2 = r->w[3 * q + 1], *w3 = r->w[3 * q + 2];
      if (sw ? tmhip_Qsw_plus_psi(ctx, w0, chi[j]) : tmhip_Qtm_plus_psi(ctx, w0, chi[j])) return 1;                                       // Y_o = Qp X_o (:96)
      if (sw ? tmhip_H_eo_sw_inv_psi(ctx, w2, chi[j], TMHIP_EO, -1, 0.) : tmhip_H_eo_tm_inv_psi(ctx, w2, chi[j], TMHIP_EO, -1.0)) return 1;   // X_e (:100,122)
      if (sw ? tmhip_H_eo_sw_inv_psi(ctx, w3, w0, TMHIP_EO, +1, 0.) : tmhip_H_eo_tm_inv_psi(ctx, w3, w0, TMHIP_EO, +1.0)) return 1;           // Y_e (:106,128)
      f[q] = rmu[j];                                                            // forcefactor = 1 (:81)
      l1[q] = w0; k1[q] = w2;                                                   // deriv_Sb(OE, w0, w2) (:124)
      l0[q] = w3; k0[q] = chi[j];                                               // deriv_Sb(EO, w3, X_o) (:130)
    }
    if (tmhip_deriv_Sb_batch(ctx, TMHIP_OE, g, l1, k1, f) || tmhip_deriv_Sb_batch(ctx, TMHIP_EO, g, l0, k0, f)) return 1;
    if (sw && G == 1) {          // :113,116: EE (w2, w3), OO (w0, X_o)
      if (tmhip_sw_spinor_eo(ctx, 0, k1[0], l0[0], f[0]) || tmhip_sw_spinor_eo(ctx, 1, l1[0], k0[0], f[0])) return 1;
    } else if (sw) {
      if (tmhip_sw_spinor_eo_batch(ctx, 0, g, k1, l0, f) || tmhip_sw_spinor_eo_batch(ctx, 1, g, l1, k0, f)) return 1;
    }
  }
  return 0;
}

// the clover monomial: refused before any launch unless sw and the inverse sw_invert(EE, 0.) made are those of the current links
static int cloverrat_prepare(tmhip_ctx *ctx, const char *who, int np) {
  if (rat_prepare(ctx, who, np)) return 1;
  if (!ctx->clover_set) TMHIP_FAIL("%s: sw_inv is not valid: call tmhip_sw_term and tmhip_sw_invert(EE, 0.) on the current links", who);
  if (ctx->sw_inv_ieo != 0 || ctx->sw_inv_mu != 0.0)
    TMHIP_FAIL("%s: sw_inv is not the one of tmhip_sw_invert(EE, 0.) (%s)", who, ctx->sw_inv_ieo < 0 ? "uploaded with tmhip_set_clover" : "other parity or mu != 0");
  if (!ctx->gauge_raw_valid) TMHIP_FAIL("%s: no lexicographic links on the device: the clover term must come from tmhip_sw_term, not tmhip_set_clover", who);
  return 0;
}
// rat_monomial.c:66-73 before the loop, :134-139 after it
static int cloverrat_force_all(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np, double kappa, double c_sw, int trlog) {
  if (tmhip_swpm_zero(ctx)) return 1;
  if (rat_force_body(ctx, chi, rmu, np, true)) return 1;
  if (trlog && tmhip_sw_deriv(ctx, 0, 0.)) return 1;
  return tmhip_sw_all(ctx, nullptr, kappa, c_sw);
}

static int rat_check_fields(const char *who, tmhip_field *const *a, tmhip_field *const *b, int n) {
  for (int j = 0; j < n; j++)
    if (!rat_eo(a[j]) || (b && !rat_eo(b[j]))) TMHIP_FAIL("%s needs fp64 one-parity (EO) fields", who);
  return 0;
}

extern "C" {

int tmhip_deriv_Sb_batch(tmhip_ctx *ctx, int ieo, int n, tmhip_field **l, tmhip_field **k, const double *factor) {
  if (n < 1 || n > RAT_MAX_PAIRS) TMHIP_FAIL("deriv_Sb_batch: n = %d is outside [1, %d]", n, RAT_MAX_PAIRS);
  if (!l || !k || !factor) TMHIP_FAIL("deriv_Sb_batch: null argument");
  for (int j = 0; j < n; j++) {
    if (!rat_eo(l[j]) || !rat_eo(k[j])) TMHIP_FAIL("deriv_Sb_batch needs fp64 one-parity fields (pair %d)", j);
    if (l[j]->ns != l[0]->ns || k[j]->ns != l[0]->ns) TMHIP_FAIL("deriv_Sb_batch: fields with different strides (pair %d)", j);
  }
  if (!ctx->gauge_set) TMHIP_FAIL("deriv_Sb_batch called before tmhip_set_gauge");
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("deriv_Sb_batch: unsplit lattices only (nproc_t = %d%s)", ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->deriv && tmhip_derivative_zero(ctx)) return 1;
  BatchArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < n; j++) { a.l[j] = l[j]->d; a.k[j] = k[j]->d; a.fac[j] = 2. * factor[j]; }
  a.g = ctx->gauge; a.deriv = ctx->deriv;
  a.n = n; a.ns = l[0]->ns; a.gs = ctx->gs; a.Vh = ctx->Vh; a.T = ctx->g.T; a.LX = ctx->g.LX; a.LY = ctx->g.LY; a.LZ = ctx->g.LZ; a.ieo = ieo ? 1 : 0;
  for (int mu = 0; mu < 4; mu++) { a.ka[mu][0] = ctx->ka[mu][0]; a.ka[mu][1] = ctx->ka[mu][1]; }
  const dim3 grid((ctx->Vh + 127) / 128, 2);
  hipLaunchKernelGGL(deriv_Sb_batch_kernel, grid, dim3(128), 0, ctx->stream, a);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_ndrat_force(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev) {
  if (rat_prepare(ctx, "ndrat_force", np)) return 1;
  if (!mu || !rmu || !chi_up || !chi_dn) TMHIP_FAIL("ndrat_force: null argument");
  if (rat_check_fields("ndrat_force", chi_up, chi_dn, np)) return 1;
  return ndrat_force_body(ctx, chi_up, chi_dn, mu, rmu, np, invmaxev);
}

int tmhip_ndrat_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, double invmaxev,
                           int max_iter, double eps_sq, int rel_prec, int *iters) {
  if (rat_prepare(ctx, "ndrat_derivative", np)) return 1;
  if (!mu || !rmu || !iters || !rat_eo(pf_up) || !rat_eo(pf_dn)) TMHIP_FAIL("ndrat_derivative: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->chi_dn, np)) return 1;
  if (tmhip_nd_mms_solve(ctx, r->chi_up, r->chi_dn, pf_up, pf_dn, mu, np, max_iter, eps_sq, rel_prec, TMHIP_ND_OP_QTM_PM, iters)) return 1;   // :107-111
  return ndrat_force_body(ctx, r->chi_up, r->chi_dn, mu, rmu, np, invmaxev);
}

static int ndrat_heatbath_body(tmhip_ctx *ctx, bool sw, tmhip_field *pf_up, tmhip_field *pf_dn, const double *nu, const double *rnu, int np, double invmaxev,
                               int max_iter, double eps_sq, int rel_prec, double *energy0, int *iters) {
  if (sw ? ndcloverrat_prepare(ctx, "ndcloverrat_heatbath", np) : rat_prepare(ctx, "ndrat_heatbath", np)) return 1;
  if (!nu || !rnu || !iters || !energy0 || !rat_eo(pf_up) || !rat_eo(pf_dn)) TMHIP_FAIL("ndrat_heatbath: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->chi_dn, np) || rat_need(ctx, r->w, 2)) return 1;
  double ea, eb;
  if (tmhip_square_norm(ctx, pf_up, ctx->Vh, 1, &ea) || tmhip_square_norm(ctx, pf_dn, ctx->Vh, 1, &eb)) return 1;   // :214,217
  *energy0 = ea + eb;
  if (tmhip_nd_mms_solve(ctx, r->chi_up, r->chi_dn, pf_up, pf_dn, nu, np, max_iter, eps_sq, rel_prec, sw ? TMHIP_ND_OP_QSW_PM : TMHIP_ND_OP_QTM_PM, iters)) return 1;   // :232
  for (int j = np - 1; j >= 0; j--) {   // pf += i rnu_j (Q_h tau^1 - i nu_j) chi_j   (:239-254)
    if (sw ? tmhip_Qsw_tau1_sub_const_ndpsi(ctx, r->w[0], r->w[1], r->chi_up[j], r->chi_dn[j], 0.0, nu[j], 1.0, invmaxev)
           : tmhip_Q_tau1_sub_const_ndpsi(ctx, r->w[0], r->w[1], r->chi_up[j], r->chi_dn[j], 0.0, nu[j], 1.0, invmaxev)) return 1;
    if (tmhip_assign_add_mul(ctx, pf_up, r->w[0], 0.0, rnu[j], ctx->Vh) || tmhip_assign_add_mul(ctx, pf_dn, r->w[1], 0.0, rnu[j], ctx->Vh)) return 1;
  }
  return 0;
}

static int ndrat_acc_body(tmhip_ctx *ctx, bool sw, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, int max_iter,
                          double eps_sq, int rel_prec, double *energy1, int *iters) {
  if (sw ? ndcloverrat_prepare(ctx, "ndcloverrat_acc", np) : rat_prepare(ctx, "ndrat_acc", np)) return 1;
  if (!mu || !rmu || !iters || !energy1 || !rat_eo(pf_up) || !rat_eo(pf_dn)) TMHIP_FAIL("ndrat_acc: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->chi_dn, np) || rat_need(ctx, r->w, 2)) return 1;
  if (tmhip_nd_mms_solve(ctx, r->chi_up, r->chi_dn, pf_up, pf_dn, mu, np, max_iter, eps_sq, rel_prec, sw ? TMHIP_ND_OP_QSW_PM : TMHIP_ND_OP_QTM_PM, iters)) return 1;   // :295
  if (tmhip_assign(ctx, r->w[0], pf_up, ctx->Vh) || tmhip_assign(ctx, r->w[1], pf_dn, ctx->Vh)) return 1;                // :299-300
  for (int j = np - 1; j >= 0; j--)                                                                                        // :301-306
    if (tmhip_assign_add_mul_r(ctx, r->w[0], r->chi_up[j], rmu[j], ctx->Vh) || tmhip_assign_add_mul_r(ctx, r->w[1], r->chi_dn[j], rmu[j], ctx->Vh)) return 1;
  double ea, eb;
  if (tmhip_scalar_prod_r(ctx, pf_up, r->w[0], ctx->Vh, 1, &ea) || tmhip_scalar_prod_r(ctx, pf_dn, r->w[1], ctx->Vh, 1, &eb)) return 1;   // :308-309
  *energy1 = ea + eb;
  return 0;
}

int tmhip_ndrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *nu, const double *rnu, int np, double invmaxev,
                         int max_iter, double eps_sq, int rel_prec, double *energy0, int *iters) {
  return ndrat_heatbath_body(ctx, false, pf_up, pf_dn, nu, rnu, np, invmaxev, max_iter, eps_sq, rel_prec, energy0, iters);
}
int tmhip_ndrat_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, int max_iter,
                    double eps_sq, int rel_prec, double *energy1, int *iters) {
  return ndrat_acc_body(ctx, false, pf_up, pf_dn, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, iters);
}

/* ---- type NDCLOVERRAT: the same bodies on the clover doublet, plus the clover part of the force ---- */
int tmhip_ndcloverrat_force(tmhip_ctx *ctx, tmhip_field **chi_up, tmhip_field **chi_dn, const double *mu, const double *rmu, int np, double invmaxev,
                            double kappa, double c_sw, int trlog) {
  if (ndcloverrat_prepare(ctx, "ndcloverrat_force", np)) return 1;
  if (!mu || !rmu || !chi_up || !chi_dn) TMHIP_FAIL("ndcloverrat_force: null argument");
  if (rat_check_fields("ndcloverrat_force", chi_up, chi_dn, np)) return 1;
  return ndcloverrat_force_all(ctx, chi_up, chi_dn, mu, rmu, np, invmaxev, kappa, c_sw, trlog);
}

int tmhip_ndcloverrat_derivative(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, double invmaxev,
                                 double kappa, double c_sw, int trlog, int max_iter, double eps_sq, int rel_prec, int *iters) {
  if (ndcloverrat_prepare(ctx, "ndcloverrat_derivative", np)) return 1;
  if (!mu || !rmu || !iters || !rat_eo(pf_up) || !rat_eo(pf_dn)) TMHIP_FAIL("ndcloverrat_derivative: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->chi_dn, np)) return 1;
  if (tmhip_cg_mms_tm_nd_op(ctx, r->chi_up, r->chi_dn, pf_up, pf_dn, mu, np, max_iter, eps_sq, rel_prec, TMHIP_ND_OP_QSW_PM, iters)) return 1;   // :106-112
  return ndcloverrat_force_all(ctx, r->chi_up, r->chi_dn, mu, rmu, np, invmaxev, kappa, c_sw, trlog);
}

int tmhip_ndcloverrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *nu, const double *rnu, int np, double invmaxev,
                               int max_iter, double eps_sq, int rel_prec, double *energy0, int *iters) {
  return ndrat_heatbath_body(ctx, true, pf_up, pf_dn, nu, rnu, np, invmaxev, max_iter, eps_sq, rel_prec, energy0, iters);
}
int tmhip_ndcloverrat_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, int np, int max_iter,
                          double eps_sq, int rel_prec, double *energy1, int *iters) {
  return ndrat_acc_body(ctx, true, pf_up, pf_dn, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, iters);
}

int tmhip_rat_force(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np) {
  if (rat_prepare(ctx, "rat_force", np)) return 1;
  if (!rmu || !chi) TMHIP_FAIL("rat_force: null argument");
  if (rat_check_fields("rat_force", chi, nullptr, np)) return 1;
  RatMuZero z(ctx);
  return rat_force_body(ctx, chi, rmu, np);
}

int tmhip_rat_derivative(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                         int *iters) {
  if (rat_prepare(ctx, "rat_derivative", np)) return 1;
  if (!mu || !rmu || !iters || !rat_eo(pf)) TMHIP_FAIL("rat_derivative: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np)) return 1;
  RatMuZero z(ctx);
  if (tmhip_cg_mms_tm(ctx, r->chi_up, pf, mu, np, max_iter, eps_sq, rel_prec, ctx->Vh, TMHIP_OP_QTM_PM, iters, nullptr)) return 1;   // :92
  return rat_force_body(ctx, r->chi_up, rmu, np);
}

static int rat_heatbath_body(tmhip_ctx *ctx, bool sw, tmhip_field *pf, const double *nu, const double *rnu, int np, int max_iter, double eps_sq, int rel_prec,
                            double *energy0, int *iters) {
  if (sw ? cloverrat_prepare(ctx, "cloverrat_heatbath", np) : rat_prepare(ctx, "rat_heatbath", np)) return 1;
  if (!nu || !rnu || !iters || !energy0 || !rat_eo(pf)) TMHIP_FAIL("%s: null argument or not an fp64 one-parity field", sw ? "cloverrat_heatbath" : "rat_heatbath");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->w, 1)) return 1;
  RatMuZero z(ctx, sw);
  if (tmhip_square_norm(ctx, pf, ctx->Vh, 1, energy0)) return 1;                                                                      // :177
  if (tmhip_cg_mms_tm(ctx, r->chi_up, pf, nu, np, max_iter, eps_sq, rel_prec, ctx->Vh, sw ? TMHIP_OP_QSW_PM : TMHIP_OP_QTM_PM, iters, nullptr)) return 1;   // :188
  for (int j = np - 1; j >= 0; j--) {   // pf += i rnu_j (Q - i nu_j) chi_j   (:194-199)
    if (sw ? tmhip_Qsw_plus_psi(ctx, r->w[0], r->chi_up[j]) : tmhip_Qtm_plus_psi(ctx, r->w[0], r->chi_up[j])) return 1;
    if (tmhip_assign_add_mul(ctx, r->w[0], r->chi_up[j], 0.0, -nu[j], ctx->Vh)) return 1;
    if (tmhip_assign_add_mul(ctx, pf, r->w[0], 0.0, rnu[j], ctx->Vh)) return 1;
  }
  return 0;
}

int tmhip_rat_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *nu, const double *rnu, int np, int max_iter, double eps_sq, int rel_prec,
                       double *energy0, int *iters) {
  return rat_heatbath_body(ctx, false, pf, nu, rnu, np, max_iter, eps_sq, rel_prec, energy0, iters);
}

static int rat_acc_body(tmhip_ctx *ctx, bool sw, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                        double *energy1, int *iters) {
  if (sw ? cloverrat_prepare(ctx, "cloverrat_acc", np) : rat_prepare(ctx, "rat_acc", np)) return 1;
  if (!mu || !rmu || !iters || !energy1 || !rat_eo(pf)) TMHIP_FAIL("%s: null argument or not an fp64 one-parity field", sw ? "cloverrat_acc" : "rat_acc");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np) || rat_need(ctx, r->w, 1)) return 1;
  RatMuZero z(ctx, sw);
  if (tmhip_cg_mms_tm(ctx, r->chi_up, pf, mu, np, max_iter, eps_sq, rel_prec, ctx->Vh, sw ? TMHIP_OP_QSW_PM : TMHIP_OP_QTM_PM, iters, nullptr)) return 1;   // :240
  if (tmhip_assign(ctx, r->w[0], pf, ctx->Vh)) return 1;                                                                              // :244
  for (int j = np - 1; j >= 0; j--)
    if (tmhip_assign_add_mul_r(ctx, r->w[0], r->chi_up[j], rmu[j], ctx->Vh)) return 1;                                                // :245-248
  return tmhip_scalar_prod_r(ctx, pf, r->w[0], ctx->Vh, 1, energy1);                                                                  // :250
}
int tmhip_rat_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                  double *energy1, int *iters) {
  return rat_acc_body(ctx, false, pf, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, iters);
}

/* ---- type CLOVERRAT (rat_monomial.c): the same bodies on the clover operators at twisted mass 0, plus the clover part of the force ---- */
int tmhip_cloverrat_force(tmhip_ctx *ctx, tmhip_field **chi, const double *rmu, int np, double kappa, double c_sw, int trlog) {
  if (cloverrat_prepare(ctx, "cloverrat_force", np)) return 1;
  if (!rmu || !chi) TMHIP_FAIL("cloverrat_force: null argument");
  if (rat_check_fields("cloverrat_force", chi, nullptr, np)) return 1;
  RatMuZero z(ctx, true);
  return cloverrat_force_all(ctx, chi, rmu, np, kappa, c_sw, trlog);
}
int tmhip_cloverrat_derivative(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, double kappa, double c_sw, int trlog,
                               int max_iter, double eps_sq, int rel_prec, int *iters) {
  if (cloverrat_prepare(ctx, "cloverrat_derivative", np)) return 1;
  if (!mu || !rmu || !iters || !rat_eo(pf)) TMHIP_FAIL("cloverrat_derivative: null argument or not an fp64 one-parity field");
  TmhipRat *r = (TmhipRat *)ctx->rat;
  if (rat_need(ctx, r->chi_up, np)) return 1;
  RatMuZero z(ctx, true);
  if (tmhip_cg_mms_tm(ctx, r->chi_up, pf, mu, np, max_iter, eps_sq, rel_prec, ctx->Vh, TMHIP_OP_QSW_PM, iters, nullptr)) return 1;   // :92
  return cloverrat_force_all(ctx, r->chi_up, rmu, np, kappa, c_sw, trlog);
}
int tmhip_cloverrat_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *nu, const double *rnu, int np, int max_iter, double eps_sq, int rel_prec,
                             double *energy0, int *iters) {
  return rat_heatbath_body(ctx, true, pf, nu, rnu, np, max_iter, eps_sq, rel_prec, energy0, iters);
}
int tmhip_cloverrat_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, int np, int max_iter, double eps_sq, int rel_prec,
                        double *energy1, int *iters) {
  return rat_acc_body(ctx, true, pf, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, iters);
}

}  // extern "C"

// ---------------------------------------------------------------- correction monomials: RATCOR / CLOVERRATCOR (monomial/ratcor_monomial.c)
// and NDRATCOR / NDCLOVERRATCOR (monomial/ndratcor_monomial.c)
// Z = Q^2 (A R)^2 - 1 with R phi = phi + sum_j rmu_j chi_j: two multi-shift solves on the stored solutions, then either the reference's
// call sequence on the single kernels ("ratcor_fused" 0: 2 np + 2 assign_add_mul_r passes, mul_r, diff and the square_norm per flavour) or
// one rat_sum launch per application of R (the second with the factor A^2 folded in) and one diff_sqnorm launch with one
// synchronisation (linalg.hip) -- both kernels reproduce the single calls bit for bit, so the two paths return the same delta and fields.
// Work fields: w[0..5] are the reference's w_fields[0..5], w[6], w[7] stand for g_chi_up/dn_spinor_field[np].
//
// The series loops of the reference run to i < 8 over coefs[6]: a seventh application of Z would read past the table.  The bodies here
// apply Z at most six times and fail, naming delta and accprec, when the sixth still leaves delta >= accprec.
static_assert(TMHIP_RAT_SUM_MAX == MSHIFT_MAX_SHIFTS, "tmhip_rat_sum carries one pointer per shift of the multi-shift solvers");
static const double ratcor_hb_coefs[6] = {1. / 4., -3. / 32., 7. / 128., -77. / 2048., 231. / 8192., -1463. / 65536.};   // ratcor_monomial.c:64, ndratcor_monomial.c:70
static const double ratcor_acc_coefs[6] = {-1. / 2., 3. / 8., -5. / 16., 35. / 128., -63. / 256., 231. / 1024.};         // ratcor_monomial.c:128, ndratcor_monomial.c:141

// the doublet bodies run with g_mu3 = 0 (ndratcor_monomial.c:73,144): the context's mu3 is put back on every path out
struct RatMu3Zero {
  tmhip_ctx *ctx; double mu3;
  explicit RatMu3Zero(tmhip_ctx *c) : ctx(c), mu3(c->mu3) { c->mu3 = 0.0; }
  ~RatMu3Zero() { ctx->mu3 = mu3; }
};

// nd: both flavours (the _dn arguments are used), op: TMHIP_OP_QTM_PM / TMHIP_OP_QSW_PM, with nd TMHIP_ND_OP_QTM_PM / TMHIP_ND_OP_QSW_PM
struct RatcorZ { bool nd; int op; const double *mu, *rmu; double A; int np, max_iter; double eps_sq; int rel_prec; };

// the fields of these entry points are one-parity fields (rat_eo, in the argument checks that follow)
static int ratcor_op_check(tmhip_ctx *ctx, const char *who, bool nd, int op, int np) {
  if (nd ? tmhip_nd_op_check(ctx, who, op) : tmhip_op_check(ctx, who, TMHIP_S_RATCOR, op, TMHIP_FIELD_EO)) return 1;
  if (!(nd ? tmhip_nd_op_row_of(op) : tmhip_op_row_of(op))->clover) return rat_prepare(ctx, who, np);
  return nd ? ndcloverrat_prepare(ctx, who, np) : cloverrat_prepare(ctx, who, np);
}

// ratcor_monomial.c:183-218 / ndratcor_monomial.c:202-245; k = Z l, *delta = |k|^2, *it0 = the first solve's return value
static int ratcor_apply_Z(tmhip_ctx *ctx, const RatcorZ &z, tmhip_field *k_up, tmhip_field *k_dn, tmhip_field *l_up, tmhip_field *l_dn, double *delta, int *it0) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  const int N = ctx->Vh, np = z.np;
  if (rat_need(ctx, r->chi_up, np) || (z.nd && rat_need(ctx, r->chi_dn, np)) || rat_need(ctx, r->w + 6, z.nd ? 2 : 1)) return 1;
  tmhip_field *t_up = r->w[6], *t_dn = r->w[7];
  const double A2 = z.A * z.A;
  int it1;
  auto solve = [&](tmhip_field *q_up, tmhip_field *q_dn, int *it) {
    return z.nd ? tmhip_nd_mms_solve(ctx, r->chi_up, r->chi_dn, q_up, q_dn, z.mu, np, z.max_iter, z.eps_sq, z.rel_prec, z.op, it)
                : tmhip_cg_mms_tm(ctx, r->chi_up, q_up, z.mu, np, z.max_iter, z.eps_sq, z.rel_prec, N, z.op, it, nullptr);
  };
  auto Qsq = [&]() { return z.nd ? tmhip_apply_nd_op(ctx, z.op, k_up, k_dn, t_up, t_dn) : tmhip_apply_op(ctx, z.op, k_up, t_up); };   // :209 / :236-237
  if (solve(l_up, l_dn, it0)) return 1;                                                       // :188 / :208
  if (ctx->opt_ratcor_fused) {
    if (tmhip_rat_sum_nd(ctx, k_up, z.nd ? k_dn : nullptr, l_up, z.nd ? l_dn : nullptr, r->chi_up, z.nd ? r->chi_dn : nullptr, z.rmu, np, 1.0)) return 1;
    if (solve(k_up, k_dn, &it1)) return 1;
    if (tmhip_rat_sum_nd(ctx, t_up, z.nd ? t_dn : nullptr, k_up, z.nd ? k_dn : nullptr, r->chi_up, z.nd ? r->chi_dn : nullptr, z.rmu, np, A2)) return 1;
    if (Qsq()) return 1;
    return tmhip_diff_sqnorm_nd(ctx, k_up, z.nd ? k_dn : nullptr, l_up, z.nd ? l_dn : nullptr, delta);
  }
  auto addR = [&]() {   // :193-196, 201-204 / :214-219, 225-230
    for (int j = np - 1; j >= 0; j--) {
      if (tmhip_assign_add_mul_r(ctx, k_up, r->chi_up[j], z.rmu[j], N)) return 1;
      if (z.nd && tmhip_assign_add_mul_r(ctx, k_dn, r->chi_dn[j], z.rmu[j], N)) return 1;
    }
    return 0;
  };
  if (tmhip_assign(ctx, k_up, l_up, N) || (z.nd && tmhip_assign(ctx, k_dn, l_dn, N))) return 1;   // :192 / :212-213
  if (addR()) return 1;
  if (solve(k_up, k_dn, &it1)) return 1;                                                      // :199 / :222
  if (addR()) return 1;
  if (tmhip_mul_r(ctx, t_up, A2, k_up, N) || (z.nd && tmhip_mul_r(ctx, t_dn, A2, k_dn, N))) return 1;   // :205 / :231-234
  if (Qsq()) return 1;
  if (tmhip_diff(ctx, k_up, k_up, l_up, N) || (z.nd && tmhip_diff(ctx, k_dn, k_dn, l_dn, N))) return 1;   // :211 / :238-239
  double a, b = 0.0;
  if (tmhip_square_norm(ctx, k_up, N, 1, &a) || (z.nd && tmhip_square_norm(ctx, k_dn, N, 1, &b))) return 1;   // :212 / :240
  *delta = z.nd ? a + b : a;
  return 0;
}

static int ratcor_args_check(const char *who, bool nd, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, const void *e, const void *napp,
                             const void *iters) {
  if (!mu || !rmu || !e || !napp || !iters || !rat_eo(pf_up) || (nd && !rat_eo(pf_dn))) TMHIP_FAIL("%s: null argument or not an fp64 one-parity field", who);
  if (nd && pf_up->d == pf_dn->d) TMHIP_FAIL("%s: the two flavours share a field", who);
  return 0;
}
static int ratcor_not_converged(const char *who, double delta, double accprec) {
  TMHIP_FAIL("%s: delta = %.6e is not below accprec = %.6e after the six applications of Z the coefficient table allows", who, delta, accprec);
}

// ratcor_monomial.c:85-110 / ndratcor_monomial.c:88-123 without the random numbers: pf holds eta on entry
static int ratcor_heatbath_body(tmhip_ctx *ctx, const char *who, const RatcorZ &z, tmhip_field *pf_up, tmhip_field *pf_dn, double accprec, double *energy0,
                                int *napp, int *iters) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  const int N = ctx->Vh;
  if (rat_need(ctx, r->w, z.nd ? 4 : 3)) return 1;
  double ea, eb = 0.0, delta = 0.0;
  if (tmhip_square_norm(ctx, pf_up, N, 1, &ea) || (z.nd && tmhip_square_norm(ctx, pf_dn, N, 1, &eb))) return 1;   // :87 / :90,93
  *energy0 = z.nd ? ea + eb : ea;
  *napp = 0; *iters = 0;
  if (tmhip_assign(ctx, r->w[0], pf_up, N) || (z.nd && tmhip_assign(ctx, r->w[1], pf_dn, N))) return 1;          // :99 / :110-111
  tmhip_field *up0 = r->w[0], *dn0 = r->w[1], *up1 = r->w[2], *dn1 = r->w[3];
  for (int i = 1; i <= 6; i++) {                                                                                  // :103-110 / :115-123
    int it0;
    if (ratcor_apply_Z(ctx, z, up1, dn1, up0, dn0, &delta, &it0)) return 1;
    *napp += 1; *iters += it0;
    if (tmhip_assign_add_mul_r(ctx, pf_up, up1, ratcor_hb_coefs[i - 1], N) || (z.nd && tmhip_assign_add_mul_r(ctx, pf_dn, dn1, ratcor_hb_coefs[i - 1], N))) return 1;
    if (delta < accprec) return 0;
    tmhip_field *t = up0; up0 = up1; up1 = t;
    t = dn0; dn0 = dn1; dn1 = t;
  }
  return ratcor_not_converged(who, delta, accprec);
}

// ratcor_monomial.c:151-168 / ndratcor_monomial.c:166-187
static int ratcor_acc_body(tmhip_ctx *ctx, const char *who, const RatcorZ &z, tmhip_field *pf_up, tmhip_field *pf_dn, double accprec, double *energy1, int *napp,
                           int *iters) {
  TmhipRat *r = (TmhipRat *)ctx->rat;
  const int N = ctx->Vh;
  if (rat_need(ctx, r->w, 6)) return 1;
  double ea, eb = 0.0, delta = 0.0;
  int it0;
  *napp = 0; *iters = 0;
  if (tmhip_assign(ctx, r->w[4], pf_up, N) || (z.nd && tmhip_assign(ctx, r->w[5], pf_dn, N))) return 1;          // :152 / :167-168
  tmhip_field *up0 = r->w[0], *dn0 = r->w[1], *up1 = r->w[2], *dn1 = r->w[3];
  if (ratcor_apply_Z(ctx, z, up0, dn0, pf_up, pf_dn, &delta, &it0)) return 1;                                     // :156 / :172
  *napp = 1; *iters = it0;
  if (tmhip_assign_add_mul_r(ctx, r->w[4], up0, ratcor_acc_coefs[0], N) || (z.nd && tmhip_assign_add_mul_r(ctx, r->w[5], dn0, ratcor_acc_coefs[0], N))) return 1;
  for (int i = 2; i <= 6; i++) {                                                                                  // :159-166 / :176-184
    if (delta < accprec) break;
    if (ratcor_apply_Z(ctx, z, up1, dn1, up0, dn0, &delta, &it0)) return 1;
    *napp += 1; *iters += it0;
    if (tmhip_assign_add_mul_r(ctx, r->w[4], up1, ratcor_acc_coefs[i - 1], N) || (z.nd && tmhip_assign_add_mul_r(ctx, r->w[5], dn1, ratcor_acc_coefs[i - 1], N))) return 1;
    tmhip_field *t = up0; up0 = up1; up1 = t;
    t = dn0; dn0 = dn1; dn1 = t;
  }
  if (!(delta < accprec)) return ratcor_not_converged(who, delta, accprec);
  if (tmhip_scalar_prod_r(ctx, pf_up, r->w[4], N, 1, &ea) || (z.nd && tmhip_scalar_prod_r(ctx, pf_dn, r->w[5], N, 1, &eb))) return 1;   // :168 / :186-187
  *energy1 = z.nd ? ea + eb : ea;
  return 0;
}

extern "C" {

int tmhip_apply_Z(tmhip_ctx *ctx, tmhip_field *k, tmhip_field *l, const double *mu, const double *rmu, double A, int np, int max_iter, double eps_sq,
                  int rel_prec, int op, double *delta, int *iters) {
  if (ratcor_op_check(ctx, "apply_Z", false, op, np)) return 1;
  if (!mu || !rmu || !delta || !iters || !rat_eo(k) || !rat_eo(l)) TMHIP_FAIL("apply_Z: null argument or not an fp64 one-parity field");
  if (k->d == l->d) TMHIP_FAIL("apply_Z: k is l (l is read again after k has been written)");
  const RatcorZ z = {false, op, mu, rmu, A, np, max_iter, eps_sq, rel_prec};
  return ratcor_apply_Z(ctx, z, k, nullptr, l, nullptr, delta, iters);
}

int tmhip_apply_Z_nd(tmhip_ctx *ctx, tmhip_field *k_up, tmhip_field *k_dn, tmhip_field *l_up, tmhip_field *l_dn, const double *mu, const double *rmu, double A,
                     int np, int max_iter, double eps_sq, int rel_prec, int op, double *delta, int *iters) {
  if (ratcor_op_check(ctx, "apply_Z_nd", true, op, np)) return 1;
  if (!mu || !rmu || !delta || !iters || !rat_eo(k_up) || !rat_eo(k_dn) || !rat_eo(l_up) || !rat_eo(l_dn)) TMHIP_FAIL("apply_Z_nd: null argument or not an fp64 one-parity field");
  if (k_up->d == l_up->d || k_up->d == l_dn->d || k_dn->d == l_up->d || k_dn->d == l_dn->d || k_up->d == k_dn->d)
    TMHIP_FAIL("apply_Z_nd: k is l or the two flavours of k share a field (l is read again after k has been written)");
  const RatcorZ z = {true, op, mu, rmu, A, np, max_iter, eps_sq, rel_prec};
  return ratcor_apply_Z(ctx, z, k_up, k_dn, l_up, l_dn, delta, iters);
}

int tmhip_ratcor_heatbath(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, double A, int np, int max_iter, double accprec, int rel_prec,
                          int op, double *energy0, int *napp, int *iters) {
  const char *who = op == TMHIP_OP_QSW_PM ? "cloverratcor_heatbath" : "ratcor_heatbath";
  if (ratcor_op_check(ctx, who, false, op, np) || ratcor_args_check(who, false, pf, nullptr, mu, rmu, energy0, napp, iters)) return 1;
  RatMuZero mz(ctx, true);   // ratcor_monomial.c:67-68
  const RatcorZ z = {false, op, mu, rmu, A, np, max_iter, accprec, rel_prec};
  return ratcor_heatbath_body(ctx, who, z, pf, nullptr, accprec, energy0, napp, iters);
}

int tmhip_ratcor_acc(tmhip_ctx *ctx, tmhip_field *pf, const double *mu, const double *rmu, double A, int np, int max_iter, double accprec, int rel_prec, int op,
                     double *energy1, int *napp, int *iters) {
  const char *who = op == TMHIP_OP_QSW_PM ? "cloverratcor_acc" : "ratcor_acc";
  if (ratcor_op_check(ctx, who, false, op, np) || ratcor_args_check(who, false, pf, nullptr, mu, rmu, energy1, napp, iters)) return 1;
  RatMuZero mz(ctx, true);   // ratcor_monomial.c:131-132
  const RatcorZ z = {false, op, mu, rmu, A, np, max_iter, accprec, rel_prec};
  return ratcor_acc_body(ctx, who, z, pf, nullptr, accprec, energy1, napp, iters);
}

int tmhip_ndratcor_heatbath(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, double A, int np, int max_iter,
                            double accprec, int rel_prec, int op, double *energy0, int *napp, int *iters) {
  const char *who = op == TMHIP_ND_OP_QSW_PM ? "ndcloverratcor_heatbath" : "ndratcor_heatbath";
  if (ratcor_op_check(ctx, who, true, op, np) || ratcor_args_check(who, true, pf_up, pf_dn, mu, rmu, energy0, napp, iters)) return 1;
  RatMu3Zero mz(ctx);   // ndratcor_monomial.c:73
  const RatcorZ z = {true, op, mu, rmu, A, np, max_iter, accprec, rel_prec};
  return ratcor_heatbath_body(ctx, who, z, pf_up, pf_dn, accprec, energy0, napp, iters);
}

int tmhip_ndratcor_acc(tmhip_ctx *ctx, tmhip_field *pf_up, tmhip_field *pf_dn, const double *mu, const double *rmu, double A, int np, int max_iter,
                       double accprec, int rel_prec, int op, double *energy1, int *napp, int *iters) {
  const char *who = op == TMHIP_ND_OP_QSW_PM ? "ndcloverratcor_acc" : "ndratcor_acc";
  if (ratcor_op_check(ctx, who, true, op, np) || ratcor_args_check(who, true, pf_up, pf_dn, mu, rmu, energy1, napp, iters)) return 1;
  RatMu3Zero mz(ctx);   // ndratcor_monomial.c:144
  const RatcorZ z = {true, op, mu, rmu, A, np, max_iter, accprec, rel_prec};
  return ratcor_acc_body(ctx, who, z, pf_up, pf_dn, accprec, energy1, napp, iters);
}

}  // extern "C"
