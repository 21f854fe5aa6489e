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
//
// mixed_cg_mms_tm_nd (solver/mixed_cg_mms_tm_nd.c) is the fp32 multi-shift CG on the same operator: the shift recurrences of mshift.h with the
// reliable-update bookkeeping behind them in one device state, one-block alpha / beta kernels, a residual kernel for shift 0 and ONE vector
// kernel for x_s and d_s of all shifts (mms32_xd_kernel; option "mms32_fused" 0 runs it as an x pass and a d pass).  The device decides a
// reliable update, the host does it after its poll (mms32_solve).
#include "hopping_common.h"
#include "cg_common.h"
#include "nd_common.h"
#include "mshift.h"

namespace {
TMHIP_SCALAR_COMPLEX_OPS(v2f, float)
#include "spinor32_io.inc"

enum { ND_EE_INV = 0, ND_OO = 1, ND_OO_DOT = 2, ND_OO_DOT_SIG = 3 /* out += sigma p before the sum: the shifted operator of the multi-shift solver */ };

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
  float mu, eps, nrm, scale, sigma;
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
    if (EPI == ND_OO_DOT || EPI == ND_OO_DOT_SIG) {
      v2f ps[6], pc[6];
      ld6<false>(ps, a.p_s, ns, i, b); ld6<false>(pc, a.p_c, ns, i, b);
      if (EPI == ND_OO_DOT_SIG) {       // assign_add_mul_r_32(Ad, d, (float) sigma[0], N)   (mixed_cg_mms_tm_nd.c:278-279)
#pragma unroll
        for (int c = 0; c < 6; c++) {
          os[c] = v2f{__builtin_fmaf(a.sigma, ps[c].x, os[c].x), __builtin_fmaf(a.sigma, ps[c].y, os[c].y)};
          oc[c] = v2f{__builtin_fmaf(a.sigma, pc[c].x, oc[c].x), __builtin_fmaf(a.sigma, pc[c].y, oc[c].y)};
        }
      }
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
  if (EPI == ND_OO_DOT || EPI == ND_OO_DOT_SIG) tmhip_wave_partial(d, a.partials, blockIdx.x * (BS / 64) + (int)(threadIdx.x >> 6));
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
  if (EPI == ND_OO_DOT || EPI == ND_OO_DOT_SIG) tmhip_wave_partial(d, a.partials, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
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
// ---------------------------------------------------------------- mixed_cg_mms_tm_nd (solver/mixed_cg_mms_tm_nd.c): state and kernels
// The shift recurrences are MshiftState's (mshift.h; normsq is the reference's rr_old), the reliable-update bookkeeping of :166-173 rides
// behind it.  zita[0] is never written and stays 0, as the reference's calloc leaves it: an update triggered by shift 0 therefore sets
// res0[0] = maxres[0] = 0 (:437-439) and shift 0 never triggers again.
struct Mms32State {
  MshiftState m;
  double res[MSHIFT_MAX_SHIFTS], res0[MSHIFT_MAX_SHIFTS], maxres[MSHIFT_MAX_SHIFTS];
  double r0r0, rel_delta;
  int check_rel;           // rel_prec != 0   (:84-91)
  int stop;                // what the host polls: the stopping test fired (m.done) or a reliable update is wanted (rel)
  int rel, rel_it;         // a reliable update was decided in iteration rel_it; every kernel enqueued behind that iteration is a no-op
  int trigger;             // trigger_shift
  int nrel, ndrop;         // reliable updates done, shifts removed
  int drop_it;             // the iteration whose check removed shift m.active (-1: none yet)
};

// The element operations, written once with their contractions spelled out: whichever kernel runs them, the bits are the same.
__device__ __forceinline__ v4f mms32_axpy(float a, v4f d, v4f x) {          // x + a d          assign_add_mul_r_32
  return v4f{__builtin_fmaf(a, d.x, x.x), __builtin_fmaf(a, d.y, x.y), __builtin_fmaf(a, d.z, x.z), __builtin_fmaf(a, d.w, x.w)};
}
__device__ __forceinline__ v4f mms32_dnew(float b, v4f d, float z, v4f r) {  // b d + z r        assign_mul_add_mul_r_32; z = 1: assign_mul_add_r_32
  return v4f{__builtin_fmaf(b, d.x, z * r.x), __builtin_fmaf(b, d.y, z * r.y), __builtin_fmaf(b, d.z, z * r.z), __builtin_fmaf(b, d.w, z * r.w)};
}

// dAd = <d, (A + sigma_0) d> from the stencil's partials, rounded to float like every fp32 sum, then alpha and the zita / alpha recurrences
// (:283-288, :317-323; the recurrences do not depend on |r|^2, so they may run ahead of the stopping test)
__global__ __launch_bounds__(256) void mms32_alpha_kernel(Mms32State *st, const double *partials, int n) {
  __shared__ double ws[4];
  const double pro = tmhip_block_sum256(partials, n, ws);
  if (threadIdx.x != 0 || st->stop) return;
  mshift_alpha_step(&st->m, (double)(float)pro);
}

// r += (float) -alphas[0] Ad and the partials of |r|^2, one per wave   (:292-298)
__global__ __launch_bounds__(256) void mms32_r_kernel(const Mms32State *st, v4f *__restrict__ r_up, v4f *__restrict__ r_dn, const v4f *__restrict__ a_up,
                                                      const v4f *__restrict__ a_dn, int ns, int N, double *part_r) {
  if (st->stop) return;   // block-uniform
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const float c = (float)-st->m.alphas[0];
  double d = 0.0;
  if (i < N) {
#pragma unroll 2
    for (int pl = 0; pl < 6; pl++) {
      const size_t o = (size_t)pl * ns + i;
      const v4f ru = mms32_axpy(c, a_up[o], r_up[o]), rd = mms32_axpy(c, a_dn[o], r_dn[o]);
      r_up[o] = ru; r_dn[o] = rd;
      d += la_dot(ru, ru) + la_dot(rd, rd);
    }
  }
  tmhip_wave_partial(d, part_r, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
}

// |r|^2, the stopping test (:307), the reliable-update decision (:326-334) and, unless an update was decided, the betas (:350-351, :359)
__global__ __launch_bounds__(256) void mms32_beta_kernel(Mms32State *st, const double *part_r, int n, int iteration) {
  __shared__ double ws[4];
  const double sum = tmhip_block_sum256(part_r, n, ws);
  if (threadIdx.x != 0 || st->stop) return;
  MshiftState *m = &st->m;
  const double rr = (double)(float)sum;
  m->err = rr;
  m->it = iteration;
  if (st->check_rel ? rr <= m->eps_sq * st->r0r0 : rr <= m->eps_sq) { m->done = 1; m->done_it = iteration; m->conv = 1; st->stop = 1; return; }
  st->res[0] = rr;
  for (int im = 1; im < m->active; im++) st->res[im] = rr * m->zita[im];
  int rel = 0;
  for (int im = m->active - 1; im >= 0; im--) {
    if (st->res[im] > st->maxres[im]) st->maxres[im] = st->res[im];
    if (st->res[im] < st->rel_delta * st->res0[im] && st->res0[im] <= st->maxres[im]) rel = 1;
    if (rel && st->trigger == -1) st->trigger = im;
  }
  if (rel) { st->rel = 1; st->rel_it = iteration; st->stop = 1; return; }
  const double b0 = rr / m->normsq;
  m->betas[0] = b0;
  m->normsq = rr;
  for (int im = 1; im < m->active; im++) m->betas[im] = b0 * m->zita[im] * m->alphas[im] / (m->zitam1[im] * m->alphas[0]);
}

// The vector pass of the shifts.  tab[4 s + 0 / 1] = x_up[s] / x_dn[s], tab[4 s + 2 / 3] = d_up[s] / d_dn[s] (the layout of TmhipNd::tab);
// blockIdx.y = s, blockIdx.z = a pair of the six float4 planes, one thread does both flavours of a site in them.  want & 1: x_s += (float) alphas[s] d_s (:340-347); want & 2:
// d_s = (float) betas[s] d_s + (float) zita[s] r, shift 0 with zita = 1 (:354-361), and on a check iteration the partials of |d_last|^2
// of the NEW d (:447-448).  want = 3 does both in one pass over x_s and d_s: four field passes per shift and flavour instead of six.
// In the iteration that decided a reliable update only the x part runs (:370-377), in every later one nothing.
__global__ __launch_bounds__(256) void mms32_xd_kernel(const Mms32State *st, v4f *const *tab, const v4f *__restrict__ r_up, const v4f *__restrict__ r_dn,
                                                       int ns, int N, double *part_sn, int want, int check, int iteration) {
  const int s = blockIdx.y;
  if (st->m.done || s >= st->m.active) return;   // block-uniform, as everything below that depends on the state
  if (st->rel) {
    if (st->rel_it != iteration) return;
    want &= 1;
  }
  if (!want) return;
  const bool do_x = want & 1, do_d = want & 2;
  const float al = (float)st->m.alphas[s], be = (float)st->m.betas[s], ze = s ? (float)st->m.zita[s] : 1.0f;
  v4f *xu = tab[4 * s], *xd = tab[4 * s + 1], *du = tab[4 * s + 2], *dd = tab[4 * s + 3];
  const bool sn = check && do_d && s >= 1 && s == st->m.active - 1;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  double acc = 0.0;
  if (i < N) {
    // blockIdx.z = a pair of planes: a block walks ten streams instead of sixty.  Every load of the pair is issued ahead of the first
    // store: the fields of the table may alias as far as the compiler knows, so it would not move a load across a store by itself
    const size_t o0 = (size_t)(2 * blockIdx.z) * ns + i, o1 = o0 + ns;
    v4f a0 = du[o0], b0 = dd[o0], a1 = du[o1], b1 = dd[o1];
    v4f xu0 = {}, xd0 = {}, xu1 = {}, xd1 = {}, ru0 = {}, rd0 = {}, ru1 = {}, rd1 = {};
    if (do_x) { xu0 = xu[o0]; xd0 = xd[o0]; xu1 = xu[o1]; xd1 = xd[o1]; }
    if (do_d) { ru0 = r_up[o0]; rd0 = r_dn[o0]; ru1 = r_up[o1]; rd1 = r_dn[o1]; }
    if (do_x) {
      xu[o0] = mms32_axpy(al, a0, xu0); xd[o0] = mms32_axpy(al, b0, xd0);
      xu[o1] = mms32_axpy(al, a1, xu1); xd[o1] = mms32_axpy(al, b1, xd1);
    }
    if (do_d) {
      a0 = mms32_dnew(be, a0, ze, ru0); b0 = mms32_dnew(be, b0, ze, rd0);
      a1 = mms32_dnew(be, a1, ze, ru1); b1 = mms32_dnew(be, b1, ze, rd1);
      du[o0] = a0; dd[o0] = b0; du[o1] = a1; dd[o1] = b1;
      if (sn) { acc += la_dot(a0, a0) + la_dot(b0, b0); acc += la_dot(a1, a1) + la_dot(b1, b1); }
    }
  }
  if (sn) tmhip_wave_partial(acc, part_sn, (blockIdx.z * gridDim.x + blockIdx.x) * 4 + (int)(threadIdx.x >> 6));   // one per wave, 12 nbl in all
}

// every tenth iteration: the last active shift leaves when alphas^2 |d|^2 <= eps_sq, on the updated d   (:445-453)
__global__ __launch_bounds__(256) void mms32_drop_kernel(Mms32State *st, const double *part_sn, int n, int iteration) {
  __shared__ double ws[4];
  const double sum = tmhip_block_sum256(part_sn, n, ws);
  if (threadIdx.x != 0 || st->m.done || st->rel || st->m.active <= 1) return;
  const double sn = (double)(float)sum, al = st->m.alphas[st->m.active - 1];
  if (al * al * sn <= st->m.eps_sq) { st->m.active -= 1; st->drop_it = iteration; st->ndrop += 1; }
}

// ... and its x is added to its P once   (:455-456, addto_32).  ptab[2 s + 0 / 1] = Pup[s] / Pdn[s]
__global__ __launch_bounds__(256) void mms32_addp_kernel(const Mms32State *st, v2d *const *ptab, v4f *const *tab, int ns, int N, int iteration) {
  if (st->drop_it != iteration) return;
  const int s = st->m.active, i = blockIdx.x * 256 + (int)threadIdx.x;   // the shift just removed
  if (i >= N) return;
#pragma unroll
  for (int f = 0; f < 2; f++) {
    v2d *P = ptab[2 * s + f];
    const v4f *x = tab[4 * s + f];
#pragma unroll
    for (int pl = 0; pl < 6; pl++) {
      const v4f a = x[(size_t)pl * ns + i];
      v2d *p0 = P + (size_t)(2 * pl) * ns + i, *p1 = p0 + ns;
      const v2d b = *p0, c = *p1;
      *p0 = v2d{b.x + (double)a.x, b.y + (double)a.y};
      *p1 = v2d{c.x + (double)a.z, c.y + (double)a.w};
    }
  }
}
}  // namespace

// ---------------------------------------------------------------- host side
struct TmhipNd32 {
  tmhip_field *s[6];           // operator scratch (g_spinor_field32[0..5]): [0, 1] EE outputs, [2, 3] first OO output, [4, 5] single-flavour hops (two-stencil form)
  tmhip_field *w32[8];         // rg_mixed_cg_her_nd: x, p, q, r (up, dn each)
  tmhip_field *w64[8];         //                     xhigh, phigh, qhigh, rhigh (up, dn each); allocated by the solver
  double *partials; int max_partials;   // [2][max_partials]: <p, A p> | |r|^2
  // mixed_cg_mms_tm_nd: x and d of the shifts s >= 1 (up, dn each; allocated as needed), the device state, the field tables, [2][mpart_n] block sums
  tmhip_field *mx[2 * MSHIFT_MAX_SHIFTS], *md[2 * MSHIFT_MAX_SHIFTS]; int nms;
  Mms32State *mst; v4f **mtab; v2d **mptab; double *mpart; int mpart_n;
};

void tmhip_nd32_destroy(tmhip_ctx *ctx) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  if (!n) return;
  for (int k = 0; k < 6; k++) tmhip_field_free(ctx, n->s[k]);
  for (int k = 0; k < 8; k++) { tmhip_field_free(ctx, n->w32[k]); tmhip_field_free(ctx, n->w64[k]); }
  for (int k = 0; k < n->nms; k++) { tmhip_field_free(ctx, n->mx[k]); tmhip_field_free(ctx, n->md[k]); }
  if (n->partials) (void)hipFree(n->partials);
  if (n->mst) (void)hipFree(n->mst);
  if (n->mtab) (void)hipFree(n->mtab);
  if (n->mptab) (void)hipFree(n->mptab);
  if (n->mpart) (void)hipFree(n->mpart);
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
                      float mu, float eps, float scale, const v2f *p_s = nullptr, const v2f *p_c = nullptr, int *npart = nullptr, float sigma = 0.0f) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  Nd32Args a;
  nd32_fill(a, ctx, ieo);
  a.out_s = out_s; a.out_c = out_c; a.k_s = k_s; a.k_c = k_c; a.p_s = p_s; a.p_c = p_c;
  a.mu = mu; a.eps = eps; a.nrm = (float)(1. / (1. + mu * mu - eps * eps)); a.scale = scale;   // float nrm = 1./(1.+ mu*mu - eps*eps)   (:93)
  a.partials = n->partials; a.sigma = sigma;
  if (ctx->opt_nd_fused32) {
    a.in_a = in_a; a.in_b = in_b;
    const bool b64 = tmhip_hop_block(ctx) == 64;
#define ND32_HOP(E) (b64 ? nd32_launch_hop<E, 64>(ctx, a, npart) : nd32_launch_hop<E, 256>(ctx, a, npart))
    if (epi == ND_EE_INV) ND32_HOP(ND_EE_INV);
    else if (epi == ND_OO) ND32_HOP(ND_OO);
    else if (epi == ND_OO_DOT) ND32_HOP(ND_OO_DOT);
    else ND32_HOP(ND_OO_DOT_SIG);
#undef ND32_HOP
  } else {
    v2f *ha = n->s[4]->d32, *hb = n->s[5]->d32;
    if (tmhip_launch_hopping32(ctx, ieo, ha, in_a, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    if (tmhip_launch_hopping32(ctx, ieo, hb, in_b, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    a.in_a = ha; a.in_b = hb;
    if (epi == ND_EE_INV) nd32_launch_mix<ND_EE_INV>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO) nd32_launch_mix<ND_OO>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO_DOT) nd32_launch_mix<ND_OO_DOT>(ctx, a, ctx->Vh, npart);
    else nd32_launch_mix<ND_OO_DOT_SIG>(ctx, a, ctx->Vh, npart);
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// Qtm_pm_ndpsi_32 (tm_operators_nd_32.c:215-263): four stages, the argument orders of nd_qpm (nd.hip).  l may alias k: k is last read in
// stage 2.  p: partials of <p, l> over both flavours from the last stage; shifted: l += sigma p first (the multi-shift solver's A + sigma_0).
static int nd32_qpm(tmhip_ctx *ctx, v2f *l_s, v2f *l_c, const v2f *k_s, const v2f *k_c, const v2f *p_s = nullptr, const v2f *p_c = nullptr,
                    int *npart = nullptr, bool shifted = false, float sigma = 0.0f) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  const float mb = (float)ctx->mubar, eb = (float)ctx->epsbar;
  const float scale2 = (float)((float)ctx->invmaxev * ctx->invmaxev);   // mul_r_32(.., (float) phmc_invmaxev*phmc_invmaxev, ..)   (:257-258)
  v2f *d0 = n->s[0]->d32, *d1 = n->s[1]->d32, *e0 = n->s[2]->d32, *e1 = n->s[3]->d32;
  if (nd32_stage(ctx, ND_EE_INV, TMHIP_EO, d0, d1, k_c, k_s, nullptr, nullptr, mb, eb, 1.0f)) return 1;
  if (nd32_stage(ctx, ND_OO, TMHIP_OE, e0, e1, d0, d1, k_c, k_s, -mb, -eb, 1.0f)) return 1;
  if (nd32_stage(ctx, ND_EE_INV, TMHIP_EO, d1, d0, e0, e1, nullptr, nullptr, -mb, eb, 1.0f)) return 1;
  return nd32_stage(ctx, p_s ? (shifted ? ND_OO_DOT_SIG : ND_OO_DOT) : ND_OO, TMHIP_OE, l_s, l_c, d0, d1, e1, e0, -mb, -eb, scale2, p_s, p_c, npart, sigma);
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

// ---------------------------------------------------------------- mixed_cg_mms_tm_nd
// solver/mixed_cg_mms_tm_nd.c:115-510 for a source with |Q|^2 = rr0 >= 1e-4.  The loop runs on the device; the host polls `stop` once per
// batch and, when the beta kernel decided a reliable update, does :364-442 itself and goes on behind that iteration.
static int mms32_solve(tmhip_ctx *ctx, int op, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts, int nsh,
                       int max_iter, double eps_sq, int rel_prec, double rr0, int *iters, int *nrel, int *nremoved) {
  TmhipNd32 *n = (TmhipNd32 *)ctx->nd32;
  const int N = ctx->Vh, ns = ctx->ns, nbl = (N + 255) / 256;
  for (int k = 0; k < 8; k++)
    if (!n->w32[k] && tmhip_field_alloc_prec(ctx, TMHIP_FIELD_EO, 1, &n->w32[k])) return 1;
  for (int k = 0; k < 6; k++)
    if (!n->w64[k] && tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &n->w64[k])) return 1;
  for (; n->nms < 2 * (nsh - 1); n->nms++)
    if (tmhip_field_alloc_prec(ctx, TMHIP_FIELD_EO, 1, &n->mx[n->nms]) || tmhip_field_alloc_prec(ctx, TMHIP_FIELD_EO, 1, &n->md[n->nms])) return 1;
  if (!n->mst) {
    n->mpart_n = 12 * nbl;   // |r|^2: 4 nbl; |d_last|^2: one per wave of the (nbl, 1, 3) blocks of a shift
    TMHIP_CHECK(hipMalloc((void **)&n->mst, sizeof(Mms32State)));
    TMHIP_CHECK(hipMalloc((void **)&n->mtab, (size_t)4 * MSHIFT_MAX_SHIFTS * sizeof(v4f *)));
    TMHIP_CHECK(hipMalloc((void **)&n->mptab, (size_t)2 * MSHIFT_MAX_SHIFTS * sizeof(v2d *)));
    TMHIP_CHECK(hipMalloc((void **)&n->mpart, (size_t)2 * n->mpart_n * sizeof(double)));
    TMHIP_CHECK(hipMemsetAsync(n->mpart, 0, (size_t)2 * n->mpart_n * sizeof(double), ctx->stream));
  }
  // sf32[0..7] and sf[0..5] of :179-194
  tmhip_field *x0[2] = {n->w32[0], n->w32[1]}, *d0[2] = {n->w32[2], n->w32[3]}, *Ad[2] = {n->w32[4], n->w32[5]}, *r[2] = {n->w32[6], n->w32[7]};
  tmhip_field *xd[2] = {n->w64[0], n->w64[1]}, *rd[2] = {n->w64[2], n->w64[3]}, *Ax[2] = {n->w64[4], n->w64[5]};
  tmhip_field *Q[2] = {Qup, Qdn};
  auto xs = [&](int s, int f) { return s ? n->mx[2 * s - 2 + f] : x0[f]; };
  for (int f = 0; f < 2; f++) {
    if (tmhip_assign_to_32(ctx, r[f], Q[f], N) || tmhip_assign_to_32(ctx, d0[f], Q[f], N)) return 1;   // :227-232
    if (tmhip_field_zero(ctx, x0[f]) || tmhip_field_zero(ctx, xd[f])) return 1;
    for (int s = 1; s < nsh; s++)                                                                       // :252-256
      if (tmhip_field_zero(ctx, n->mx[2 * s - 2 + f]) || tmhip_assign_to_32(ctx, n->md[2 * s - 2 + f], Q[f], N)) return 1;
    for (int s = 0; s < nsh; s++)                                                                       // :264-267
      if (tmhip_field_zero(ctx, f ? Pdn[s] : Pup[s])) return 1;
  }
  Mms32State h;
  memset(&h, 0, sizeof(h));
  h.m.sigma0 = shifts[0] * shifts[0];
  h.m.alpha0 = h.m.alphas[0] = 1.0;
  for (int s = 0; s < nsh; s++) h.res[s] = h.res0[s] = h.maxres[s] = rr0;
  for (int s = 1; s < nsh; s++) {
    h.m.sigma[s] = shifts[s] * shifts[s] - h.m.sigma0;
    h.m.zita[s] = h.m.zitam1[s] = h.m.alphas[s] = 1.0;
  }
  h.m.normsq = rr0; h.m.eps_sq = eps_sq; h.m.target = rel_prec ? eps_sq * rr0 : eps_sq;
  h.m.active = h.m.pact = nsh; h.m.max_iter = max_iter; h.m.done_it = -1;
  h.r0r0 = rr0; h.rel_delta = 1.0e-10; h.check_rel = rel_prec != 0; h.trigger = -1; h.drop_it = -1;
  v4f *tab[4 * MSHIFT_MAX_SHIFTS];
  v2d *ptab[2 * MSHIFT_MAX_SHIFTS];
  for (int s = 0; s < nsh; s++) {
    tab[4 * s] = F4(xs(s, 0)); tab[4 * s + 1] = F4(xs(s, 1));
    tab[4 * s + 2] = F4(s ? n->md[2 * s - 2] : d0[0]); tab[4 * s + 3] = F4(s ? n->md[2 * s - 1] : d0[1]);
    ptab[2 * s] = Pup[s]->d; ptab[2 * s + 1] = Pdn[s]->d;
  }
  TMHIP_CHECK(hipMemcpyAsync(n->mtab, tab, sizeof(v4f *) * 4 * nsh, hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(n->mptab, ptab, sizeof(v2d *) * 2 * nsh, hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(n->mst, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  Mms32State *st = n->mst;
  double *part_r = n->mpart, *part_sn = n->mpart + n->mpart_n;
  const float sigma0 = (float)h.m.sigma0;
  const int fused = ctx->opt_mms32_fused;
  const dim3 gs(nbl, nsh, 3), one(1), bs(256);
  auto launch_xd = [&](int want, int check, int iteration) {
    hipLaunchKernelGGL(mms32_xd_kernel, gs, bs, 0, ctx->stream, (const Mms32State *)st, (v4f *const *)n->mtab, (const v4f *)F4(r[0]), (const v4f *)F4(r[1]),
                       ns, N, part_sn, want, check, iteration);
  };
  auto launch_drop = [&](int iteration) {
    hipLaunchKernelGGL(mms32_drop_kernel, one, bs, 0, ctx->stream, st, (const double *)part_sn, 12 * nbl, iteration);
    hipLaunchKernelGGL(mms32_addp_kernel, dim3(nbl), bs, 0, ctx->stream, (const Mms32State *)st, (v2d *const *)n->mptab, (v4f *const *)n->mtab, ns, N, iteration);
  };
  auto enqueue = [&](int iteration) {
    const int check = nsh > 1 && iteration > 0 && iteration % 10 == 0;
    int np = 0;
    if (nd32_qpm(ctx, Ad[0]->d32, Ad[1]->d32, d0[0]->d32, d0[1]->d32, d0[0]->d32, d0[1]->d32, &np, true, sigma0)) return 1;   // :276-279
    hipLaunchKernelGGL(mms32_alpha_kernel, one, bs, 0, ctx->stream, st, (const double *)n->partials, np);
    hipLaunchKernelGGL(mms32_r_kernel, dim3(nbl), bs, 0, ctx->stream, (const Mms32State *)st, F4(r[0]), F4(r[1]), (const v4f *)F4(Ad[0]), (const v4f *)F4(Ad[1]),
                       ns, N, part_r);
    hipLaunchKernelGGL(mms32_beta_kernel, one, bs, 0, ctx->stream, st, (const double *)part_r, 4 * nbl, iteration);
    if (fused) launch_xd(3, check, iteration);
    else { launch_xd(1, 0, iteration); launch_xd(2, check, iteration); }
    if (check) launch_drop(iteration);
    return 0;
  };
  const int batch = ctx->opt_cg_batch > 0 ? ctx->opt_cg_batch : 4;
  int base = 0, j = max_iter;
  for (;;) {
    if (tmhip_poll_loop(ctx, max_iter - base, true, batch, 1.0e3 * h.m.target, &st->stop, &st->m.err, 0, false, [&](int k) { return enqueue(base + k); })) return 1;
    TMHIP_CHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h.m.done) { j = h.m.done_it; break; }
    if (!h.rel) break;                                   // max_iter iterations without meeting the precision
    // the reliable update of iteration rel_it; the x of that iteration were updated on the device (:370-377)
    MshiftState &m = h.m;
    for (int s = 0; s < m.active; s++)                   // :373-380
      if (tmhip_add_from_32(ctx, Pup[s], xs(s, 0), N) || tmhip_add_from_32(ctx, Pdn[s], xs(s, 1), N)) return 1;
    if (tmhip_add_from_32(ctx, xd[0], x0[0], N) || tmhip_add_from_32(ctx, xd[1], x0[1], N)) return 1;   // :383-384
    if (tmhip_apply_nd_op(ctx, op, Ax[0], Ax[1], xd[0], xd[1])) return 1;                               // :387-390
    double ru, rdn;
    for (int f = 0; f < 2; f++)
      if (tmhip_assign_add_mul_r(ctx, Ax[f], xd[f], m.sigma0, N) || tmhip_diff(ctx, rd[f], Q[f], Ax[f], N)) return 1;   // :389-393
    if (tmhip_square_norm(ctx, rd[0], N, 1, &ru) || tmhip_square_norm(ctx, rd[1], N, 1, &rdn)) return 1;
    const double rr = ru + rdn;
    h.res[0] = rr;
    // :404-408.  The reference leaves the loop here with x already added to P and adds it once more at :466-475; so does this.
    if (h.res[h.trigger] > h.res0[h.trigger] && h.trigger == 0) { j = h.rel_it; break; }
    for (int s = 0; s < m.active; s++)                   // :411-416
      if (tmhip_field_zero(ctx, xs(s, 0)) || tmhip_field_zero(ctx, xs(s, 1))) return 1;
    if (tmhip_assign_to_32(ctx, r[0], rd[0], N) || tmhip_assign_to_32(ctx, r[1], rd[1], N)) return 1;   // :419-420
    m.betas[0] = h.res[0] / m.normsq;                    // :424-425
    m.normsq = rr;
    for (int im = 1; im < m.active; im++) m.betas[im] = m.betas[0] * m.zita[im] * m.alphas[im] / (m.zitam1[im] * m.alphas[0]);   // :431
    h.res[h.trigger] = h.res[0] * m.zita[h.trigger] * m.zita[h.trigger];   // :437-441 (zita[0] = 0)
    h.res0[h.trigger] = h.maxres[h.trigger] = h.res[h.trigger];
    h.trigger = -1;
    h.nrel += 1;
    h.rel = 0; h.stop = 0;
    const int it = h.rel_it, check = nsh > 1 && it > 0 && it % 10 == 0;
    TMHIP_CHECK(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    launch_xd(2, check, it);                             // :427-434
    if (check) launch_drop(it);                          // :445-459
    TMHIP_CHECK(hipGetLastError());
    base = it + 1;
    if (base >= max_iter) {
      TMHIP_CHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
      break;
    }
  }
  for (int s = 0; s < h.m.active; s++)                   // :466-475
    if (tmhip_add_from_32(ctx, Pup[s], xs(s, 0), N) || tmhip_add_from_32(ctx, Pdn[s], xs(s, 1), N)) return 1;
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->nd_active_shifts = h.m.active;
  *iters = j < max_iter ? j : -1;                        // :505-510
  if (nrel) *nrel = h.nrel;
  if (nremoved) *nremoved = h.ndrop;
  return 0;
}

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

/* solver/mixed_cg_mms_tm_nd.c:69-511 with M_ndpsi = Qtm_pm_ndpsi, M_ndpsi32 = Qtm_pm_ndpsi_32 */
int tmhip_mixed_cg_mms_tm_nd(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts, int nshifts,
                             int max_iter, double eps_sq, int rel_prec, int op, int *iters, int *rel_updates, int *removed) {
  if (nshifts < 1 || nshifts > MSHIFT_MAX_SHIFTS) TMHIP_FAIL("mixed_cg_mms_tm_nd: nshifts = %d is outside [1, %d]", nshifts, MSHIFT_MAX_SHIFTS);
  if (!Pup || !Pdn || !shifts || !iters) TMHIP_FAIL("mixed_cg_mms_tm_nd: null argument");
  if (tmhip_nd_op_check(ctx, "mixed_cg_mms_tm_nd", op, TMHIP_S_MIXED)) return 1;
  if (ctx->g.nproc_t > 1 || ctx->loopback)
    TMHIP_FAIL("mixed_cg_mms_tm_nd: the fp32 doublet runs on unsplit lattices only (nproc_t = %d%s)", ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  if (!nd32_f64(Qup) || !nd32_f64(Qdn)) TMHIP_FAIL("mixed_cg_mms_tm_nd needs fp64 one-parity (EO) source fields");
  for (int s = 0; s < nshifts; s++) {
    if (!nd32_f64(Pup[s]) || !nd32_f64(Pdn[s])) TMHIP_FAIL("mixed_cg_mms_tm_nd needs fp64 one-parity (EO) solution fields");
    if (Pup[s]->d == Qup->d || Pup[s]->d == Qdn->d || Pdn[s]->d == Qup->d || Pdn[s]->d == Qdn->d) TMHIP_FAIL("mixed_cg_mms_tm_nd: a solution field is the source");
  }
  if (max_iter < 1) TMHIP_FAIL("mixed_cg_mms_tm_nd: max_iter < 1");
  if (nd32_prepare(ctx, "mixed_cg_mms_tm_nd")) return 1;
  double ru, rdn;
  if (tmhip_square_norm(ctx, Qup, ctx->Vh, 1, &ru) || tmhip_square_norm(ctx, Qdn, ctx->Vh, 1, &rdn)) return 1;   // :105-107
  if (ru + rdn < 1.0e-4) {                                                                                       // :110-113
    if (tmhip_cg_mms_tm_nd_op(ctx, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, op, iters)) return 1;
    if (rel_updates) *rel_updates = 0;
    if (removed) *removed = nshifts - ctx->nd_active_shifts;
    return 0;
  }
  return mms32_solve(ctx, op, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, ru + rdn, iters, rel_updates, removed);
}

}  // extern "C"

// what solver_params.type == MIXEDCGMMSND selects in monomial/ndrat_monomial.c:107,228,291 (solver/monomial_solve.c:252-268)
int tmhip_nd_mms_solve(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts, int nshifts,
                       int max_iter, double eps_sq, int rel_prec, int op, int *iters) {
  if (ctx->opt_nd_mms_mixed && op == TMHIP_ND_OP_QTM_PM)
    return tmhip_mixed_cg_mms_tm_nd(ctx, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, op, iters, nullptr, nullptr);
  return tmhip_cg_mms_tm_nd_op(ctx, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, op, iters);
}
