// The fp32 twins of the non-degenerate doublet (operator/tm_operators_nd_32.c) and the reliable-update mixed CG on them
// (solver/rg_mixed_cg_her_nd.c) on the device.
//
// nd32_hop_kernel is the fp32 twin of nd_hop_kernel (nd.hip): one thread does one output site for both flavours, each of the eight
// links is loaded ONCE and applied to the two projected half-spinors, and the site-local mixing of M_ee_inv_ndpsi_32 /
// M_oo_sub_g5_ndpsi_32 (tm_operators_nd_32.c:90-211) runs in the epilogue, so Qtm_pm_ndpsi_32 is four launches.  It reads and writes
// the packed fp32 layouts of hopping32.hip through 16-byte accesses: spinors are six float4 planes, the gauge twin ctx->gauge32 is four
// float4 planes and one float2 plane per (parity, direction).  A link is read in full (18 reals) whatever "gauge_recon" says.
// Arithmetic is in float; mu, eps, nrm and phmc_invmaxev^2 are rounded to float as the reference's casts do (:226-258).  The spin
// algebra, the mixing and the neighbour indices are those of the fp64 kernel (nd_common.h), the grid rule is nd_launch_hop's.
// Option "nd_fused" 0 builds the same operator from two tmhip_hopping_matrix_32 launches per hop plus nd32_mix_kernel, which also
// serves the stand-alone site-local calls.
//
// rg_mixed_cg_her_nd is rg_mixed_solve (cg_common.h, shared with the single-flavour solver) on pairs of fields: the scalar steps of an
// iteration are CgState's with inner = 2 / 3, the sums over the two flavours are added up before them, and the field updates of an
// iteration are the pair kernels below, in fp32 and in fp64.
#include "hopping_common.h"
#include "cg_common.h"
#include "nd_common.h"

namespace {
TMHIP_SCALAR_COMPLEX_OPS(v2f, float)
#include "spinor32_io.inc"

enum { ND_EE_INV = 0, ND_OO = 1, ND_OO_DOT = 2 };

struct Nd32Args {
  v2f *out_s, *out_c;
  const v2f *in_a, *in_b;     // stencil: accumulator a is gathered from in_a, b from in_b; nd32_mix_kernel: a, b are read at the site
  const v2f *k_s, *k_c;       // ND_OO*: the local pair that is mixed (a, b are then j_s, j_c)
  const v2f *p_s, *p_c;       // ND_OO_DOT: partial sums of <p, out> over both flavours
  double *partials;           // ND_OO_DOT: one per wave
  const v2f *gauge;           // already offset to the parity of the output sites
  int ns, gs, T, LX, LY, LZh, Vh, face, YZh, par_off;
  int nxcd_chunk, map_nb;     // > 0: blocks b, b+8, .. share an XCD and take a contiguous chunk of the lattice
  float ka[4][2];
  float mu, eps, nrm, scale;
};

// one hop of both flavours: the link is read once, five loads per lane (hopping32.hip)
template <int D, bool NT>
__device__ __forceinline__ void nd32_hop_dir(v2f (&aa)[12], v2f (&ab)[12], const v2f *__restrict__ ia, const v2f *__restrict__ ib, size_t ns, int j,
                                             const v2f *__restrict__ g, size_t gs, int i, v2f ka) {
  v2f u[9];
  const v2f *gp = g + (size_t)D * 9 * gs;
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const vf4 *q = reinterpret_cast<const vf4 *>(gp + (size_t)m * 2 * gs) + i;
    const vf4 v = NT ? __builtin_nontemporal_load(q) : *q;
    u[2 * m] = v2f{v.x, v.y}; u[2 * m + 1] = v2f{v.z, v.w};
  }
  u[8] = ldc<NT>(gp + (size_t)8 * gs + i);
  v2f s[12], pa[3], pb[3];
  ld6<false>(s, ia, ns, j, 0); ld6<false>(s + 6, ia, ns, j, 1);
  ndc::nd_project<D>(s, pa, pb);
  ndc::nd_apply<D>(aa, u, pa, pb, ka);
  ld6<false>(s, ib, ns, j, 0); ld6<false>(s + 6, ib, ns, j, 1);
  ndc::nd_project<D>(s, pa, pb);
  ndc::nd_apply<D>(ab, u, pa, pb, ka);
}

// The site-local mixing of both flavours, on a (= strange slot) and b (= charm slot), and the stores; returns this site's share of
// <p, out> (ND_OO_DOT), accumulated in double.  Written once for the fused stencil and for the mixing pass.
template <int EPI>
__device__ __forceinline__ double nd32_epilogue(const Nd32Args &a, int i, const v2f (&va)[12], const v2f (&vb)[12]) {
  const size_t ns = (size_t)a.ns;
  double d = 0.0;
#pragma unroll
  for (int b = 0; b < 2; b++) {       // spins 0, 1 | spins 2, 3
    v2f ks[6], kc[6], os[6], oc[6];
    if (EPI == ND_EE_INV) {
#pragma unroll
      for (int c = 0; c < 6; c++) { ks[c] = va[6 * b + c]; kc[c] = vb[6 * b + c]; }
    } else {
      ld6<false>(ks, a.k_s, ns, i, b); ld6<false>(kc, a.k_c, ns, i, b);
    }
    ndc::nd_mix6<EPI == ND_EE_INV>(b, a.mu, a.eps, EPI == ND_EE_INV ? a.nrm : a.scale, ks, kc, &va[6 * b], &vb[6 * b], os, oc);
    if (EPI == ND_OO_DOT) {
      v2f ps[6], pc[6];
      ld6<false>(ps, a.p_s, ns, i, b); ld6<false>(pc, a.p_c, ns, i, b);
#pragma unroll
      for (int c = 0; c < 6; c++) d += cdotd(ps[c], os[c]) + cdotd(pc[c], oc[c]);
    }
    st6<false>(a.out_s, ns, i, b, os);
    st6<false>(a.out_c, ns, i, b, oc);
  }
  return d;
}

// One thread per output site, both flavours.  Every thread reaches the end (inactive ones with d = 0), so the reducing form writes one
// partial per wave of the grid, padding blocks included: the sum never depends on the block order.  Three waves per SIMD, the floor of
// the gather kernels (tools/check_resources.py).
template <int EPI, int BS, bool NT>
__global__ __launch_bounds__(BS, 3) void nd32_hop_kernel(const Nd32Args a) {
  int bid = blockIdx.x;
  if (a.nxcd_chunk > 0) bid = (bid & 7) * a.nxcd_chunk + (bid >> 3);
  const int i = bid * BS + (int)threadIdx.x;
  double d = 0.0;
  if (bid < a.map_nb && i < a.Vh) {
    int j[8];
    ndc::nd_neighbours(a, i, j);
    v2f aa[12], ab[12];
#pragma unroll
    for (int c = 0; c < 12; c++) { aa[c] = czero(); ab[c] = czero(); }
    const v2f ka0 = v2f{a.ka[0][0], a.ka[0][1]}, ka1 = v2f{a.ka[1][0], a.ka[1][1]};
    const v2f ka2 = v2f{a.ka[2][0], a.ka[2][1]}, ka3 = v2f{a.ka[3][0], a.ka[3][1]};
    const size_t ns = (size_t)a.ns, gs = (size_t)a.gs;
    nd32_hop_dir<0, NT>(aa, ab, a.in_a, a.in_b, ns, j[0], a.gauge, gs, i, ka0);
    nd32_hop_dir<1, NT>(aa, ab, a.in_a, a.in_b, ns, j[1], a.gauge, gs, i, ka0);
    nd32_hop_dir<2, NT>(aa, ab, a.in_a, a.in_b, ns, j[2], a.gauge, gs, i, ka1);
    nd32_hop_dir<3, NT>(aa, ab, a.in_a, a.in_b, ns, j[3], a.gauge, gs, i, ka1);
    nd32_hop_dir<4, NT>(aa, ab, a.in_a, a.in_b, ns, j[4], a.gauge, gs, i, ka2);
    nd32_hop_dir<5, NT>(aa, ab, a.in_a, a.in_b, ns, j[5], a.gauge, gs, i, ka2);
    nd32_hop_dir<6, NT>(aa, ab, a.in_a, a.in_b, ns, j[6], a.gauge, gs, i, ka3);
    nd32_hop_dir<7, NT>(aa, ab, a.in_a, a.in_b, ns, j[7], a.gauge, gs, i, ka3);
    d = nd32_epilogue<EPI>(a, i, aa, ab);
  }
  if (EPI == ND_OO_DOT) tmhip_wave_partial(d, a.partials, blockIdx.x * (BS / 64) + (int)(threadIdx.x >> 6));
}

// The mixing alone, a and b read at the site: the stand-alone M_ee_inv_ndpsi_32 / M_oo_sub_g5_ndpsi_32 and the second half of the
// two-stencil form.  One partial per wave as above.
template <int EPI>
__global__ __launch_bounds__(256) void nd32_mix_kernel(const Nd32Args a, int N) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  double d = 0.0;
  if (i < N) {
    v2f va[12], vb[12];
    const size_t ns = (size_t)a.ns;
    ld6<false>(va, a.in_a, ns, i, 0); ld6<false>(va + 6, a.in_a, ns, i, 1);
    ld6<false>(vb, a.in_b, ns, i, 0); ld6<false>(vb + 6, a.in_b, ns, i, 1);
    d = nd32_epilogue<EPI>(a, i, va, vb);
  }
  if (EPI == ND_OO_DOT) tmhip_wave_partial(d, a.partials, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
}

// ---------------------------------------------------------------- the field updates of a CG iteration on a pair of fields
// V = v2d (twelve planes) or v4f (six planes of component pairs); blockIdx.y = plane, blockIdx.z = flavour.  Scalars have the element
// type, sums are accumulated in double (cg.hip's kernels on one field).
template <class V> struct Pair { V *u, *d; };
template <class V> struct CPair { const V *u, *d; };

// pro = <p, q> over both flavours   (rg_mixed_cg_her_nd.c:95,134)
template <class V>
__global__ __launch_bounds__(LA_BS) void ndcg_dot_kernel(CPair<V> P, CPair<V> Q, int ns, int N, double *partials, const CgState *st) {
  if (st->done) return;
  const size_t off = (size_t)blockIdx.y * ns;
  const V *p = (blockIdx.z ? P.d : P.u) + off, *q = (blockIdx.z ? Q.d : Q.u) + off;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) acc += la_dot(p[i], q[i]);
  }
  cg_block_reduce_store(acc, partials);
}

// x += alpha p ; r += -alpha q ; partial |r|^2   (:96-98, :136-138)
template <class V>
__global__ __launch_bounds__(LA_BS) void ndcg_update_kernel(Pair<V> X, CPair<V> P, CPair<V> Q, Pair<V> R, int ns, int N, double *partials,
                                                            const CgState *st) {
  if (st->done) return;
  typedef decltype(V{}.x) RT;
  const RT alpha = (RT)st->alpha;
  const size_t off = (size_t)blockIdx.y * ns;
  V *x = (blockIdx.z ? X.d : X.u) + off, *r = (blockIdx.z ? R.d : R.u) + off;
  const V *p = (blockIdx.z ? P.d : P.u) + off, *q = (blockIdx.z ? Q.d : Q.u) + off;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      x[i] = x[i] + alpha * p[i];
      const V c = r[i] + (-alpha) * q[i];
      r[i] = c;
      acc += la_dot(c, c);
    }
  }
  cg_block_reduce_store(acc, partials);
}

// p = beta p + r   (:101, :146)
template <class V>
__global__ __launch_bounds__(LA_BS) void ndcg_xpay_kernel(Pair<V> P, CPair<V> R, int ns, int N, const CgState *st) {
  if (st->done) return;
  typedef decltype(V{}.x) RT;
  const RT beta = (RT)st->beta;
  const size_t off = (size_t)blockIdx.y * ns;
  V *p = (blockIdx.z ? P.d : P.u) + off;
  const V *r = (blockIdx.z ? R.d : R.u) + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) p[i] = beta * p[i] + r[i];
  }
}
}  // namespace

// ---------------------------------------------------------------- host side
struct TmhipNd32 {
  tmhip_field *s[6];           // operator scratch (g_spinor_field32[0..5]): [0, 1] EE outputs, [2, 3] first OO output, [4, 5] single-flavour hops (two-stencil form)
  tmhip_field *w32[8];         // rg_mixed_cg_her_nd: x, p, q, r (up, dn each)
  tmhip_field *w64[8];         //                     xhigh, phigh, qhigh, rhigh (up, dn each); allocated by the solver
  double *partials; int max_partials;   // [2][max_partials]: <p, A p> | |r|^2
};

void tmhip_nd32_destroy(tmhip_ctx *ctx) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  if (!n) return;
  for (int k = 0; k < 6; k++) tmhip_field_free(ctx, n->s[k]);
  for (int k = 0; k < 8; k++) { tmhip_field_free(ctx, n->w32[k]); tmhip_field_free(ctx, n->w64[k]); }
  if (n->partials) (void)hipFree(n->partials);
  delete n;
  ctx->nd32 = nullptr;
}

// the fp64 doublet's rule: unsplit lattices only, and the loopback rehearsal counts as split.  Before anything is allocated or launched.
static int nd32_prepare(tmhip_ctx *ctx, const char *who) {
  if (ctx->g.nproc_t > 1 || ctx->loopback)
    TMHIP_FAIL("%s: the fp32 doublet runs on unsplit lattices only (nproc_t = %d%s)", who, ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (tmhip_prepare_fp32(ctx)) return 1;
  if (ctx->nd32) return 0;
  TmhipNd32 *n = new TmhipNd32();
  ctx->nd32 = n;
  for (int k = 0; k < 6; k++)
    if (tmhip_field_alloc_prec(ctx, TMHIP_FIELD_EO, 1, &n->s[k])) return 1;
  // stencil: one partial per wave of the padded grid (at most Vh / 64 + 32); mix kernel: 4 per block; pair kernels: 2 flavours x 12 planes
  // x one per 1024 sites (at most Vh / 42 + 24)
  n->max_partials = ctx->Vh / 32 + 64;
  TMHIP_CHECK(hipMalloc((void **)&n->partials, (size_t)2 * n->max_partials * sizeof(double)));
  return 0;
}

static bool nd32_f32(const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 1; }
static bool nd32_f64(const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 0; }

static int nd32_check4(tmhip_ctx *ctx, const char *who, tmhip_field *a, tmhip_field *b, tmhip_field *c, tmhip_field *d) {
  if (nd32_prepare(ctx, who)) return 1;
  if (!nd32_f32(a) || !nd32_f32(b) || !nd32_f32(c) || !nd32_f32(d)) TMHIP_FAIL("%s needs four fp32 one-parity (EO) fields", who);
  if (a->d32 == b->d32) TMHIP_FAIL("%s: the two output flavours must be different fields", who);
  return 0;
}

static void nd32_fill(Nd32Args &a, tmhip_ctx *ctx, int ieo) {
  memset(&a, 0, sizeof(a));
  a.gauge = ctx->gauge32 + (size_t)(ieo ? 1 : 0) * 72 * ctx->gs;
  a.ns = ctx->ns; a.gs = ctx->gs;
  a.T = ctx->g.T; a.LX = ctx->g.LX; a.LY = ctx->g.LY; a.LZh = ctx->g.LZ / 2;
  a.Vh = ctx->Vh; a.face = ctx->face; a.YZh = ctx->g.LY * ctx->g.LZ / 2;
  a.par_off = ieo & 1;
  for (int m = 0; m < 4; m++) { a.ka[m][0] = (float)ctx->ka[m][0]; a.ka[m][1] = (float)ctx->ka[m][1]; }
  a.scale = 1.0f;
}

template <int EPI, int BS>
static void nd32_launch_hop(tmhip_ctx *ctx, Nd32Args a, int *npart) {
  const int nb = ndc::nd_grid(ctx, BS, &a.map_nb, &a.nxcd_chunk);
  if (ndc::nd_gauge_cached(ctx, sizeof(v2f))) hipLaunchKernelGGL((nd32_hop_kernel<EPI, BS, false>), dim3(nb), dim3(BS), 0, ctx->stream, a);
  else hipLaunchKernelGGL((nd32_hop_kernel<EPI, BS, true>), dim3(nb), dim3(BS), 0, ctx->stream, a);
  if (npart) *npart = nb * (BS / 64);
}

template <int EPI>
static void nd32_launch_mix(tmhip_ctx *ctx, const Nd32Args &a, int N, int *npart) {
  const int nb = (N + 255) / 256;
  hipLaunchKernelGGL((nd32_mix_kernel<EPI>), dim3(nb), dim3(256), 0, ctx->stream, a, N);
  if (npart) *npart = 4 * nb;
}

// One hop of a doublet + its mixing epilogue (nd_stage of nd.hip in fp32).  mu, eps, scale arrive as the reference's floats.
static int nd32_stage(tmhip_ctx *ctx, int epi, int ieo, v2f *out_s, v2f *out_c, const v2f *in_a, const v2f *in_b, const v2f *k_s, const v2f *k_c,
                      float mu, float eps, float scale, const v2f *p_s = nullptr, const v2f *p_c = nullptr, int *npart = nullptr) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  Nd32Args a;
  nd32_fill(a, ctx, ieo);
  a.out_s = out_s; a.out_c = out_c; a.k_s = k_s; a.k_c = k_c; a.p_s = p_s; a.p_c = p_c;
  a.mu = mu; a.eps = eps; a.nrm = (float)(1. / (1. + mu * mu - eps * eps)); a.scale = scale;   // float nrm = 1./(1.+ mu*mu - eps*eps)   (:93)
  a.partials = n->partials;
  if (ctx->opt_nd_fused32) {
    a.in_a = in_a; a.in_b = in_b;
    const bool b64 = tmhip_hop_block(ctx) == 64;
#define ND32_HOP(E) (b64 ? nd32_launch_hop<E, 64>(ctx, a, npart) : nd32_launch_hop<E, 256>(ctx, a, npart))
    if (epi == ND_EE_INV) ND32_HOP(ND_EE_INV);
    else if (epi == ND_OO) ND32_HOP(ND_OO);
    else ND32_HOP(ND_OO_DOT);
#undef ND32_HOP
  } else {
    v2f *ha = n->s[4]->d32, *hb = n->s[5]->d32;
    if (tmhip_launch_hopping32(ctx, ieo, ha, in_a, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    if (tmhip_launch_hopping32(ctx, ieo, hb, in_b, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    a.in_a = ha; a.in_b = hb;
    if (epi == ND_EE_INV) nd32_launch_mix<ND_EE_INV>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO) nd32_launch_mix<ND_OO>(ctx, a, ctx->Vh, npart);
    else nd32_launch_mix<ND_OO_DOT>(ctx, a, ctx->Vh, npart);
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// Qtm_pm_ndpsi_32 (tm_operators_nd_32.c:215-263): four stages, the argument orders of nd_qpm (nd.hip).  l may alias k: k is last read in
// stage 2.  p: partials of <p, l> over both flavours from the last stage.
static int nd32_qpm(tmhip_ctx *ctx, v2f *l_s, v2f *l_c, const v2f *k_s, const v2f *k_c, const v2f *p_s = nullptr, const v2f *p_c = nullptr,
                    int *npart = nullptr) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  const float mb = (float)ctx->mubar, eb = (float)ctx->epsbar;
  const float scale2 = (float)((float)ctx->invmaxev * ctx->invmaxev);   // mul_r_32(.., (float) phmc_invmaxev*phmc_invmaxev, ..)   (:257-258)
  v2f *d0 = n->s[0]->d32, *d1 = n->s[1]->d32, *e0 = n->s[2]->d32, *e1 = n->s[3]->d32;
  if (nd32_stage(ctx, ND_EE_INV, TMHIP_EO, d0, d1, k_c, k_s, nullptr, nullptr, mb, eb, 1.0f)) return 1;
  if (nd32_stage(ctx, ND_OO, TMHIP_OE, e0, e1, d0, d1, k_c, k_s, -mb, -eb, 1.0f)) return 1;
  if (nd32_stage(ctx, ND_EE_INV, TMHIP_EO, d1, d0, e0, e1, nullptr, nullptr, -mb, eb, 1.0f)) return 1;
  return nd32_stage(ctx, p_s ? ND_OO_DOT : ND_OO, TMHIP_OE, l_s, l_c, d0, d1, e1, e0, -mb, -eb, scale2, p_s, p_c, npart);
}

// ---------------------------------------------------------------- rg_mixed_cg_her_nd
// The doublet's fields of rg_mixed_solve (cg_common.h): rg_mixed_cg_her_nd.c:222-230
struct RgNdFields {
  tmhip_ctx *ctx; int op, N;
  tmhip_field *P[2], *Q[2];
  tmhip_field *xh[2], *ph[2], *qh[2], *rh[2], *x[2], *p[2], *q[2], *r[2];
  double *pa, *pr;   // block sums of <p, A p> and |r|^2
  int each(int (*fn)(tmhip_ctx *, tmhip_field *, tmhip_field *, int), tmhip_field **a, tmhip_field **b) {
    return fn(ctx, a[0], b[0], N) || fn(ctx, a[1], b[1], N);
  }
  int norm(tmhip_field **a, double *s) {   // square_norm(up) + square_norm(dn)
    double u, d;
    if (tmhip_square_norm(ctx, a[0], N, 1, &u) || tmhip_square_norm(ctx, a[1], N, 1, &d)) return 1;
    *s = u + d;
    return 0;
  }
  int zero(tmhip_field **a) { return tmhip_field_zero(ctx, a[0]) || tmhip_field_zero(ctx, a[1]); }
  int source_norm(double *s) { return norm(Q, s); }
  int start() { return zero(x) || zero(P) || each(tmhip_assign, ph, Q) || each(tmhip_assign, rh, Q); }
  int rhigh_norm(double *s) { return norm(rh, s); }
  int restart32() { return each(tmhip_assign_to_32, r, rh) || each(tmhip_assign_to_32, p, rh); }
  int zero_x32() { return zero(x); }
  int accumulate32() { return each(tmhip_add_from_32, P, x); }
  int true_residual(double *s) {
    if (tmhip_apply_nd_op(ctx, op, qh[0], qh[1], P[0], P[1])) return 1;
    if (tmhip_diff(ctx, rh[0], Q[0], qh[0], N) || tmhip_diff(ctx, rh[1], Q[1], qh[1], N)) return 1;
    return norm(rh, s);
  }
  int restart64() { return each(tmhip_assign, ph, rh) || zero(xh); }
  int accumulate64() { return tmhip_assign_add_mul_r(ctx, P[0], xh[0], 1.0, N) || tmhip_assign_add_mul_r(ctx, P[1], xh[1], 1.0, N); }

  // one iteration: q = A p and <p, q> ; alpha ; x += alpha p, r -= alpha q, |r|^2 ; beta and the stopping test ; p = beta p + r
  int enqueue32(CgState *st) {
    double *sum = ctx->result_dev + 1;
    int np = 0;
    if (nd32_qpm(ctx, q[0]->d32, q[1]->d32, p[0]->d32, p[1]->d32, p[0]->d32, p[1]->d32, &np)) return 1;
    hipLaunchKernelGGL(cg_sum_scalar_kernel<0>, dim3(1), dim3(CG_SUM_BS), 0, ctx->stream, (const double *)pa, np, sum, st, (double *)nullptr, 0);
    dim3 g = la_grid32(N);
    g.z = 2;
    const int ns = ctx->ns;
    hipLaunchKernelGGL(ndcg_update_kernel<v4f>, g, dim3(LA_BS), 0, ctx->stream, Pair<v4f>{F4(x[0]), F4(x[1])}, CPair<v4f>{F4(p[0]), F4(p[1])},
                       CPair<v4f>{F4(q[0]), F4(q[1])}, Pair<v4f>{F4(r[0]), F4(r[1])}, ns, N, pr, (const CgState *)st);
    hipLaunchKernelGGL(cg_sum_scalar_kernel<1>, dim3(1), dim3(CG_SUM_BS), 0, ctx->stream, (const double *)pr, (int)(g.x * g.y * g.z), sum, st, (double *)nullptr, 0);
    hipLaunchKernelGGL(ndcg_xpay_kernel<v4f>, g, dim3(LA_BS), 0, ctx->stream, Pair<v4f>{F4(p[0]), F4(p[1])}, CPair<v4f>{F4(r[0]), F4(r[1])}, ns, N,
                       (const CgState *)st);
    return 0;
  }
  int enqueue64(CgState *st) {
    double *sum = ctx->result_dev + 1;
    if (tmhip_apply_nd_op(ctx, op, qh[0], qh[1], ph[0], ph[1])) return 1;
    dim3 g = la_grid(N);
    g.z = 2;
    const int ns = ctx->ns, nblk = (int)(g.x * g.y * g.z);
    hipLaunchKernelGGL(ndcg_dot_kernel<v2d>, g, dim3(LA_BS), 0, ctx->stream, CPair<v2d>{ph[0]->d, ph[1]->d}, CPair<v2d>{qh[0]->d, qh[1]->d}, ns, N, pa,
                       (const CgState *)st);
    hipLaunchKernelGGL(cg_sum_scalar_kernel<0>, dim3(1), dim3(CG_SUM_BS), 0, ctx->stream, (const double *)pa, nblk, sum, st, (double *)nullptr, 0);
    hipLaunchKernelGGL(ndcg_update_kernel<v2d>, g, dim3(LA_BS), 0, ctx->stream, Pair<v2d>{xh[0]->d, xh[1]->d}, CPair<v2d>{ph[0]->d, ph[1]->d},
                       CPair<v2d>{qh[0]->d, qh[1]->d}, Pair<v2d>{rh[0]->d, rh[1]->d}, ns, N, pr, (const CgState *)st);
    hipLaunchKernelGGL(cg_sum_scalar_kernel<1>, dim3(1), dim3(CG_SUM_BS), 0, ctx->stream, (const double *)pr, nblk, sum, st, (double *)nullptr, 0);
    hipLaunchKernelGGL(ndcg_xpay_kernel<v2d>, g, dim3(LA_BS), 0, ctx->stream, Pair<v2d>{ph[0]->d, ph[1]->d}, CPair<v2d>{rh[0]->d, rh[1]->d}, ns, N,
                       (const CgState *)st);
    return 0;
  }
  int loop32(double *rho, double delta, double eps, int base, int max_iter, int *j) {
    return rg_inner_loop(ctx, "rg_mixed_cg_her_nd", true, rho, delta, eps, base, max_iter, j, [&](CgState *st) { return enqueue32(st); });
  }
  int loop64(double *rho, double delta, double eps, int base, int max_iter, int *j) {
    return rg_inner_loop(ctx, "rg_mixed_cg_her_nd", false, rho, delta, eps, base, max_iter, j, [&](CgState *st) { return enqueue64(st); });
  }
};

extern "C" {

int tmhip_M_ee_inv_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, float mu, float eps) {
  if (nd32_check4(ctx, "M_ee_inv_ndpsi_32", l_s, l_c, k_s, k_c)) return 1;
  Nd32Args a;
  nd32_fill(a, ctx, 0);
  a.out_s = l_s->d32; a.out_c = l_c->d32; a.in_a = k_s->d32; a.in_b = k_c->d32;
  a.mu = mu; a.eps = eps; a.nrm = (float)(1. / (1. + mu * mu - eps * eps));
  nd32_launch_mix<ND_EE_INV>(ctx, a, ctx->Vh, nullptr);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_M_oo_sub_g5_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *j_s,
                               tmhip_field *j_c, float mu, float eps) {
  if (nd32_check4(ctx, "M_oo_sub_g5_ndpsi_32", l_s, l_c, k_s, k_c)) return 1;
  if (!nd32_f32(j_s) || !nd32_f32(j_c)) TMHIP_FAIL("M_oo_sub_g5_ndpsi_32 needs fp32 one-parity (EO) fields");
  Nd32Args a;
  nd32_fill(a, ctx, 0);
  a.out_s = l_s->d32; a.out_c = l_c->d32; a.in_a = j_s->d32; a.in_b = j_c->d32; a.k_s = k_s->d32; a.k_c = k_c->d32;
  a.mu = mu; a.eps = eps;
  nd32_launch_mix<ND_OO>(ctx, a, ctx->Vh, nullptr);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_Qtm_pm_ndpsi_32(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (nd32_check4(ctx, "Qtm_pm_ndpsi_32", l_s, l_c, k_s, k_c)) return 1;
  return nd32_qpm(ctx, l_s->d32, l_c->d32, k_s->d32, k_c->d32);
}

int tmhip_rg_mixed_cg_her_nd(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                             int rel_prec, int N, int op, double delta, int *iters, int *iter_out, int *iter_in_sp, int *iter_in_dp) {
  if (tmhip_nd_op_check(ctx, "rg_mixed_cg_her_nd", op, TMHIP_S_MIXED)) return 1;
  if (!iters) TMHIP_FAIL("rg_mixed_cg_her_nd: null argument");
  if (nd32_prepare(ctx, "rg_mixed_cg_her_nd")) return 1;
  if (!nd32_f64(P_up) || !nd32_f64(P_dn) || !nd32_f64(Q_up) || !nd32_f64(Q_dn)) TMHIP_FAIL("rg_mixed_cg_her_nd needs four fp64 one-parity (EO) fields");
  if (P_up->d == P_dn->d || P_up->d == Q_up->d || P_up->d == Q_dn->d || P_dn->d == Q_up->d || P_dn->d == Q_dn->d)
    TMHIP_FAIL("rg_mixed_cg_her_nd: the solution fields must differ from each other and from the source");
  if (N != ctx->Vh) TMHIP_FAIL("rg_mixed_cg_her_nd: N must be VOLUME/2");
  if (cg_state_alloc(ctx)) return 1;
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  for (int k = 0; k < 8; k++) {
    if (!n->w32[k] && tmhip_field_alloc_prec(ctx, TMHIP_FIELD_EO, 1, &n->w32[k])) return 1;
    if (!n->w64[k] && tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &n->w64[k])) return 1;
  }
  if (24 * ((N + LA_BS * LA_UNROLL - 1) / (LA_BS * LA_UNROLL)) > n->max_partials) TMHIP_FAIL("rg_mixed_cg_her_nd: partials buffer too small");
  RgNdFields f = {ctx, op, N, {P_up, P_dn}, {Q_up, Q_dn},
                  {n->w64[0], n->w64[1]}, {n->w64[2], n->w64[3]}, {n->w64[4], n->w64[5]}, {n->w64[6], n->w64[7]},
                  {n->w32[0], n->w32[1]}, {n->w32[2], n->w32[3]}, {n->w32[4], n->w32[5]}, {n->w32[6], n->w32[7]},
                  n->partials, n->partials + n->max_partials};
  return rg_mixed_solve(f, max_iter, eps_sq, rel_prec, delta, iters, iter_out, iter_in_sp, iter_in_dp);
}

}  // extern "C"
