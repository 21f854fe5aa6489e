// The non-degenerate twisted-mass doublet (operator/tm_operators_nd.c, solver/cg_her_nd.c, solver/cg_mms_tm_nd.c) on the device.
//
// A doublet is a pair of one-parity fields (strange = up, charm = dn).  Every composition of tm_operators_nd.c is a
// hop of BOTH flavours followed by a site-local mixing of the two:
//   M_ee_inv_ndpsi     (:639-696)  l_s = nrm [(1 -+ i mu) k_s + eps k_c],  l_c = nrm [(1 +- i mu) k_c + eps k_s],  nrm = 1/(1 + mu^2 - eps^2)
//   M_oo_sub_g5_ndpsi  (:698-757)  the same mixing without nrm, minus j on spins 0, 1 and j minus it on spins 2, 3
// (upper sign: spins 0, 1).  nd_hop_kernel does both flavours of a site in one thread: each of the eight links is loaded ONCE
// and applied to the two projected half-spinors, and the mixing runs in the epilogue on the two accumulators, so a
// Qtm_pm_ndpsi is four launches and nothing else.  The flavour swaps the reference writes as argument orders (tau_1) are
// pointer choices here.  Option "nd_fused" 0 builds the same operator from two single-flavour stencil launches (EPI_STORE)
// per hop plus one mixing pass (nd_mix_kernel) -- the A/B of DESIGN.md section 4.  What does not depend on the precision -- the spin
// algebra of a hop, the mixing, the neighbour indices, the grid rule -- lives in nd_common.h and serves the fp32 twin (nd32.hip) too.
//
// The solvers share one device-resident engine (nd_solve): the coefficients of the multi-shift recurrences live in a
// MshiftState and are updated by one-block kernels (the recurrences themselves: mshift.h, shared with mms.hip), the field
// updates read them from there, and the host polls `done` at batch boundaries only (tmhip_poll_loop, tmhip_internal.h).
// cg_her_nd is the one-shift, sigma = 0 case with its own start (P != 0 allowed) and return convention.
#include "hopping_common.h"
#include "mshift.h"
#include "nd_common.h"

namespace {
TMHIP_SCALAR_COMPLEX_OPS(v2d, double)
TMHIP_SPINOR_IO_PLANES

using ndc::cfma; using ndc::cfmac; using ndc::cmul; using ndc::cmulc; using ndc::nd_project; using ndc::nd_apply;   // nd_common.h

enum { ND_EE_INV = 0, ND_OO = 1, ND_OO_DOT = 2, ND_OO_SUBC = 3,
       // the clover doublet (Qsw_*_ndpsi): the same four roles, then the two halves of NDSW_EE on their own (site-local kernel only)
       NDSW_EE = 4, NDSW_OO = 5, NDSW_OO_DOT = 6, NDSW_OO_SUBC = 7, NDSW_MUL = 8, NDSW_INV = 9 };

struct NdArgs {
  v2d *out_s, *out_c;
  const v2d *in_a, *in_b;     // stencil: accumulator a is gathered from in_a, b from in_b; nd_mix_kernel: a, b are read at the site
  const v2d *k_s, *k_c;       // ND_OO*: the local pair that is mixed (a, b are then j_s, j_c)
  const v2d *p_s, *p_c;       // ND_OO_DOT: out += sigma p, partial sums of <p, out> over both flavours
  double *partials;           // ND_OO_DOT: one per wave (stencil) / per block (mix kernel)
  const v2d *gauge;           // already offset to the parity of the output sites
  int ns, gs, T, LX, LY, LZh, Vh, face, YZh, par_off;
  int nxcd_chunk, map_nb;     // > 0: blocks b, b+8, .. share an XCD and take a contiguous chunk of the lattice
  double ka[4][2];
  double mu, eps, nrm, scale, sigma;
  const v2d *sw, *swi;       // NDSW_*: 1+T of the output sites' parity [6][9][gs], sw_inv_nd [8][9][gs] (block 2a + chirality)
  double cz[2];              // ND_OO_SUBC: out -= cz (.) the OTHER flavour's k (Q_tau1_sub_const_ndpsi: its k arrive swapped)
};

// one hop of both flavours: the link is read once
template <int D, bool NT>
__device__ __forceinline__ void nd_hop_dir(v2d (&aa)[12], v2d (&ab)[12], const v2d *__restrict__ ia, const v2d *__restrict__ ib, size_t ns, int j,
                                           const v2d *__restrict__ g, size_t gs, int i, v2d ka) {
  v2d u[9];
  const v2d *gd = g + (size_t)D * 9 * gs + i;
#pragma unroll
  for (int e = 0; e < 9; e++) u[e] = ldc<NT>(gd + (size_t)e * gs);
  v2d s[12], pa[3], pb[3];
  ld6<false>(s, ia, ns, j, 0); ld6<false>(s + 6, ia, ns, j, 1);
  nd_project<D>(s, pa, pb);
  nd_apply<D>(aa, u, pa, pb, ka);
  ld6<false>(s, ib, ns, j, 0); ld6<false>(s + 6, ib, ns, j, 1);
  nd_project<D>(s, pa, pb);
  nd_apply<D>(ab, u, pa, pb, ka);
}

// The site-local mixing of both flavours, on a (= strange slot) and b (= charm slot), and the stores; returns this site's
// share of <p, out> (ND_OO_DOT).  Written once for the fused stencil and for the mixing pass of the two-stencil form.
template <int EPI>
__device__ __forceinline__ double nd_epilogue(const NdArgs &a, int i, const v2d (&va)[12], const v2d (&vb)[12]) {
  const size_t ns = (size_t)a.ns;
  const double mu = a.mu, eps = a.eps;
  double d = 0.0;
#pragma unroll
  for (int b = 0; b < 2; b++) {       // spins 0, 1 | spins 2, 3
    v2d ks[6], kc[6], os[6], oc[6];
    if (EPI == ND_EE_INV) {
#pragma unroll
      for (int c = 0; c < 6; c++) { ks[c] = va[6 * b + c]; kc[c] = vb[6 * b + c]; }
    } else {
      ld6<false>(ks, a.k_s, ns, i, b); ld6<false>(kc, a.k_c, ns, i, b);
    }
    ndc::nd_mix6<EPI == ND_EE_INV>(b, mu, eps, EPI == ND_EE_INV ? a.nrm : a.scale, ks, kc, &va[6 * b], &vb[6 * b], os, oc);
    if (EPI == ND_OO_SUBC) {          // l_strange -= Cpol z k_strange, l_charm -= Cpol z k_charm (tm_operators_nd.c:349-374); k_s, k_c hold (k_charm, k_strange)
      const v2d cz = v2d{a.cz[0], a.cz[1]};
#pragma unroll
      for (int c = 0; c < 6; c++) { os[c] = os[c] - cmul(cz, kc[c]); oc[c] = oc[c] - cmul(cz, ks[c]); }
    }
    if (EPI == ND_OO_DOT) {           // the shifted operator of cg_mms_tm_nd.c:120-124 and its (p, A p) over both flavours
      v2d ps[6], pc[6];
      ld6<false>(ps, a.p_s, ns, i, b); ld6<false>(pc, a.p_c, ns, i, b);
#pragma unroll
      for (int c = 0; c < 6; c++) {
        os[c] = os[c] + a.sigma * ps[c];
        oc[c] = oc[c] + a.sigma * pc[c];
        d += cdotd(ps[c], os[c]) + cdotd(pc[c], oc[c]);
      }
    }
    st6<false>(a.out_s, ns, i, b, os);
    st6<false>(a.out_c, ns, i, b, oc);
  }
  return d;
}

// ---------------------------------------------------------------- clover doublet: site-local arithmetic
// The 6x6 blocks are streamed one 3x3 at a time and one chirality at a time; a block is read once and applied to both flavours.
__device__ __forceinline__ void ndsw_ld(v2d (&u)[9], const v2d *__restrict__ w, size_t gs, int i, int blk) {
#pragma unroll
  for (int e = 0; e < 9; e++) u[e] = w[((size_t)blk * 9 + e) * gs + i];
}
template <bool DAG, bool ACC>
__device__ __forceinline__ void ndsw_mv(v2d *r, const v2d (&u)[9], const v2d *x) {   // r (+)= U x or U^dagger x
#pragma unroll
  for (int row = 0; row < 3; row++) {
    const v2d t = ACC ? r[row] : czero();
    if (DAG) r[row] = cfmac(u[6 + row], x[2], cfmac(u[3 + row], x[1], cfmac(u[row], x[0], t)));
    else r[row] = cfma(u[3 * row + 2], x[2], cfma(u[3 * row + 1], x[1], cfma(u[3 * row], x[0], t)));
  }
}
// assign_mul_one_sw_pm_imu_eps (clovertm_operators.c:960-1074) on chirality b, ADDED to what oa / ob hold on entry (zero, or minus
// the hopped pair for clover_gamma5_nd: the accumulators' registers are free before the block products start):
//   oa += (1+T) xa + i m xa + eps xb,  ob += (1+T) xb - i m xb + eps xa,   m = mu on spins 0, 1 and -mu on spins 2, 3.
// a = the reference's "_s" arguments, b = its "_c" arguments.
__device__ __forceinline__ void ndsw_mul(const v2d *__restrict__ sw, size_t gs, int i, int b, double mu, double eps, const v2d *xa, const v2d *xb,
                                         v2d *oa, v2d *ob) {
  const double m = b == 0 ? mu : -mu;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    oa[c] = oa[c] + v2d{-m * xa[c].y, m * xa[c].x} + eps * xb[c];
    ob[c] = ob[c] + v2d{m * xb[c].y, -m * xb[c].x} + eps * xa[c];
  }
  v2d u[9];
  ndsw_ld(u, sw, gs, i, 0 + b);                                          // sw[x][0][b]
  ndsw_mv<false, true>(oa, u, xa); ndsw_mv<false, true>(ob, u, xb);
  ndsw_ld(u, sw, gs, i, 2 + b);                                          // sw[x][1][b] and its dagger
  ndsw_mv<false, true>(oa, u, xa + 3); ndsw_mv<false, true>(ob, u, xb + 3);
  ndsw_mv<true, true>(oa + 3, u, xa); ndsw_mv<true, true>(ob + 3, u, xb);
  ndsw_ld(u, sw, gs, i, 4 + b);                                          // sw[x][2][b]
  ndsw_mv<false, true>(oa + 3, u, xa + 3); ndsw_mv<false, true>(ob + 3, u, xb + 3);
}
// clover_inv_nd (clovertm_operators.c:352-425) on chirality b: the same four blocks of sw_inv_nd on both flavours
__device__ __forceinline__ void ndsw_inv(const v2d *__restrict__ swi, size_t gs, int i, int b, const v2d *xa, const v2d *xb, v2d *oa, v2d *ob) {
  v2d u[9];
  ndsw_ld(u, swi, gs, i, 0 + b);
  ndsw_mv<false, false>(oa, u, xa); ndsw_mv<false, false>(ob, u, xb);
  ndsw_ld(u, swi, gs, i, 2 + b);
  ndsw_mv<false, true>(oa, u, xa + 3); ndsw_mv<false, true>(ob, u, xb + 3);
  ndsw_ld(u, swi, gs, i, 6 + b);
  ndsw_mv<false, false>(oa + 3, u, xa); ndsw_mv<false, false>(ob + 3, u, xb);
  ndsw_ld(u, swi, gs, i, 4 + b);
  ndsw_mv<false, true>(oa + 3, u, xa + 3); ndsw_mv<false, true>(ob + 3, u, xb + 3);
}

// The clover twin of nd_epilogue, on va (= the "_s" slot) and vb (= the "_c" slot).
//   NDSW_EE  : out = sw_inv_nd [(1+T) v +- i mu v + eps v']                      (assign_mul_one_sw_pm_imu_eps, then clover_inv_nd)
//   NDSW_OO* : out = scale g5 [(1+T) k +- i mu k + eps k' - v]                   (clover_gamma5_nd :733-850, then mul_r)
//   NDSW_MUL / NDSW_INV: the two halves of NDSW_EE on their own
template <int EPI>
__device__ __forceinline__ double ndsw_epilogue(const NdArgs &a, int i, const v2d (&va)[12], const v2d (&vb)[12]) {
  const size_t ns = (size_t)a.ns, gs = (size_t)a.gs;
  double d = 0.0;
#pragma unroll
  for (int b = 0; b < 2; b++) {       // spins 0, 1 | spins 2, 3
    v2d os[6], oc[6];
    if (EPI == NDSW_EE || EPI == NDSW_MUL) {
#pragma unroll
      for (int c = 0; c < 6; c++) os[c] = oc[c] = czero();
      ndsw_mul(a.sw, gs, i, b, a.mu, a.eps, &va[6 * b], &vb[6 * b], os, oc);
      if (EPI == NDSW_EE) {
        v2d ts[6], tc[6];
#pragma unroll
        for (int c = 0; c < 6; c++) { ts[c] = os[c]; tc[c] = oc[c]; }
        ndsw_inv(a.swi, gs, i, b, ts, tc, os, oc);
      }
    } else if (EPI == NDSW_INV) {
      ndsw_inv(a.swi, gs, i, b, &va[6 * b], &vb[6 * b], os, oc);
    } else {
      v2d ks[6], kc[6];
      ld6<false>(ks, a.k_s, ns, i, b); ld6<false>(kc, a.k_c, ns, i, b);
#pragma unroll
      for (int c = 0; c < 6; c++) { os[c] = -va[6 * b + c]; oc[c] = -vb[6 * b + c]; }
      ndsw_mul(a.sw, gs, i, b, a.mu, a.eps, ks, kc, os, oc);
      const double g5s = b == 0 ? a.scale : -a.scale;   // gamma5, then mul_r
#pragma unroll
      for (int c = 0; c < 6; c++) { os[c] = g5s * os[c]; oc[c] = g5s * oc[c]; }
      if (EPI == NDSW_OO_SUBC) {      // out -= Cpol z (the OTHER slot's k): Qsw_tau1_sub_const_ndpsi's outputs arrive swapped (tm_operators_nd.c:401-441)
        const v2d cz = v2d{a.cz[0], a.cz[1]};
#pragma unroll
        for (int c = 0; c < 6; c++) { os[c] = os[c] - cmul(cz, kc[c]); oc[c] = oc[c] - cmul(cz, ks[c]); }
      }
      if (EPI == NDSW_OO_DOT) {
        v2d ps[6], pc[6];
        ld6<false>(ps, a.p_s, ns, i, b); ld6<false>(pc, a.p_c, ns, i, b);
#pragma unroll
        for (int c = 0; c < 6; c++) {
          os[c] = os[c] + a.sigma * ps[c];
          oc[c] = oc[c] + a.sigma * pc[c];
          d += cdotd(ps[c], os[c]) + cdotd(pc[c], oc[c]);
        }
      }
    }
    st6<false>(a.out_s, ns, i, b, os);
    st6<false>(a.out_c, ns, i, b, oc);
  }
  return d;
}
template <int EPI>
__device__ __forceinline__ double nd_epilogue_any(const NdArgs &a, int i, const v2d (&va)[12], const v2d (&vb)[12]) {
  if constexpr (EPI >= NDSW_EE) return ndsw_epilogue<EPI>(a, i, va, vb);
  else return nd_epilogue<EPI>(a, i, va, vb);
}
constexpr bool nd_epi_dot(int epi) { return epi == ND_OO_DOT || epi == NDSW_OO_DOT; }

// One thread per output site, both flavours.  Every thread reaches the end (inactive ones with d = 0), so the reducing form
// writes one partial per wave of the grid, padding blocks included: the sum never depends on the block order.
template <int EPI, int BS, bool NT>
__device__ __forceinline__ void nd_hop_body(const NdArgs a) {
  int bid = blockIdx.x;
  if (a.nxcd_chunk > 0) bid = (bid & 7) * a.nxcd_chunk + (bid >> 3);
  const int i = bid * BS + (int)threadIdx.x;
  double d = 0.0;
  if (bid < a.map_nb && i < a.Vh) {
    int j[8];
    ndc::nd_neighbours(a, i, j);
    v2d aa[12], ab[12];
#pragma unroll
    for (int c = 0; c < 12; c++) { aa[c] = czero(); ab[c] = czero(); }
    const v2d ka0 = cbcast(a.ka[0][0], a.ka[0][1]), ka1 = cbcast(a.ka[1][0], a.ka[1][1]);
    const v2d ka2 = cbcast(a.ka[2][0], a.ka[2][1]), ka3 = cbcast(a.ka[3][0], a.ka[3][1]);
    const size_t ns = (size_t)a.ns, gs = (size_t)a.gs;
    nd_hop_dir<0, NT>(aa, ab, a.in_a, a.in_b, ns, j[0], a.gauge, gs, i, ka0);
    nd_hop_dir<1, NT>(aa, ab, a.in_a, a.in_b, ns, j[1], a.gauge, gs, i, ka0);
    nd_hop_dir<2, NT>(aa, ab, a.in_a, a.in_b, ns, j[2], a.gauge, gs, i, ka1);
    nd_hop_dir<3, NT>(aa, ab, a.in_a, a.in_b, ns, j[3], a.gauge, gs, i, ka1);
    nd_hop_dir<4, NT>(aa, ab, a.in_a, a.in_b, ns, j[4], a.gauge, gs, i, ka2);
    nd_hop_dir<5, NT>(aa, ab, a.in_a, a.in_b, ns, j[5], a.gauge, gs, i, ka2);
    nd_hop_dir<6, NT>(aa, ab, a.in_a, a.in_b, ns, j[6], a.gauge, gs, i, ka3);
    nd_hop_dir<7, NT>(aa, ab, a.in_a, a.in_b, ns, j[7], a.gauge, gs, i, ka3);
    d = nd_epilogue_any<EPI>(a, i, aa, ab);
  }
  if (nd_epi_dot(EPI)) tmhip_wave_partial(d, a.partials, blockIdx.x * (BS / 64) + (int)(threadIdx.x >> 6));
}
template <int EPI, int BS, bool NT>
__global__ __launch_bounds__(BS) void nd_hop_kernel(const NdArgs a) { nd_hop_body<EPI, BS, NT>(a); }
// the clover epilogues stream two 6x6 block products per flavour and chirality on top of the stencil: held to two waves per SIMD,
// the floor of the single-flavour clover kernels (tools/check_resources.py)
template <int EPI, int BS, bool NT>
__global__ __launch_bounds__(BS, 2) void ndsw_hop_kernel(const NdArgs a) { nd_hop_body<EPI, BS, NT>(a); }

// The mixing alone, a and b read at the site: the standalone M_ee_inv_ndpsi / M_oo_sub_g5_ndpsi and the second half of the
// two-stencil form.  One partial per wave as above.
template <int EPI>
__device__ __forceinline__ void nd_mix_body(const NdArgs a, int N) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  double d = 0.0;
  if (i < N) {
    v2d va[12], vb[12];
    const size_t ns = (size_t)a.ns;
    ld6<false>(va, a.in_a, ns, i, 0); ld6<false>(va + 6, a.in_a, ns, i, 1);
    ld6<false>(vb, a.in_b, ns, i, 0); ld6<false>(vb + 6, a.in_b, ns, i, 1);
    d = nd_epilogue_any<EPI>(a, i, va, vb);
  }
  if (nd_epi_dot(EPI)) tmhip_wave_partial(d, a.partials, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
}
template <int EPI>
__global__ __launch_bounds__(256) void nd_mix_kernel(const NdArgs a, int N) { nd_mix_body<EPI>(a, N); }
template <int EPI>
__global__ __launch_bounds__(256, 2) void ndsw_mix_kernel(const NdArgs a, int N) { nd_mix_body<EPI>(a, N); }

// ---------------------------------------------------------------- solver state and kernels
// pro = <p, (A + sigma0) p> over both flavours (the stencil's ND_OO_DOT partials), then the alpha step
__global__ __launch_bounds__(256) void nd_alpha_kernel(MshiftState *st, const double *partials, int n) {
  __shared__ double ws[4];
  const double pro = tmhip_block_sum256(partials, n, ws);
  if (threadIdx.x != 0 || st->done) return;
  mshift_alpha_step(st, pro);
}

// field table of the shifts: tab[4 s + 0 / 1] = P_up[s] / P_dn[s], tab[4 s + 2 / 3] = ps_up[s] / ps_dn[s] (shift 0: the x and p of the CG)
// blockIdx.y = s.  s = 0: x += alphas[0] p, r -= alphas[0] A p, partials of |r|^2 (cg_mms_tm_nd.c:170-180);
// s >= 1 (active): P[s] += alphas[s] ps[s] (:149-150), and on a check iteration the last active shift adds up |ps|^2 (:158-160)
__global__ __launch_bounds__(256) void nd_x_kernel(MshiftState *st, v2d *const *tab, v2d *r_up, v2d *r_dn, const v2d *ap_up, const v2d *ap_dn,
                                                   int ns, int N, double *part_r, double *part_sn, int check) {
  const int s = blockIdx.y;
  if (st->done || s >= st->active) return;   // block-uniform
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const double al = st->alphas[s];
  v2d *xu = tab[4 * s], *xd = tab[4 * s + 1];
  const v2d *pu = tab[4 * s + 2], *pd = tab[4 * s + 3];
  double d = 0.0;
  const bool sn = check && s >= 1 && s == st->active - 1;
  if (i < N) {
#pragma unroll 4
    for (int c = 0; c < 12; c++) {
      const size_t o = (size_t)c * ns + i;
      const v2d a = pu[o], b = pd[o];
      xu[o] = xu[o] + al * a;
      xd[o] = xd[o] + al * b;
      if (s == 0) {
        const v2d ru = r_up[o] + (-al) * ap_up[o], rd = r_dn[o] + (-al) * ap_dn[o];
        r_up[o] = ru; r_dn[o] = rd;
        d += cdotd(ru, ru) + cdotd(rd, rd);
      } else if (sn) {
        d += cdotd(a, a) + cdotd(b, b);
      }
    }
  }
  if (s == 0) tmhip_wave_partial(d, part_r, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  else if (sn) tmhip_wave_partial(d, part_sn, blockIdx.x * 4 + (int)(threadIdx.x >> 6));
}

// |r|^2 and, on a check iteration, |ps_last|^2, then the beta step
__global__ __launch_bounds__(256) void nd_beta_kernel(MshiftState *st, const double *part_r, const double *part_sn, int n, int check, int iteration) {
  __shared__ double ws[4];
  const double err = tmhip_block_sum256(part_r, n, ws);
  __syncthreads();
  const double sn = check ? tmhip_block_sum256(part_sn, n, ws) : 0.0;
  if (threadIdx.x != 0 || st->done) return;
  mshift_beta_step(st, err, sn, check, iteration);
}

// p = beta p + r (s = 0, :193-194), ps[s] = betas[s] ps[s] + zita[s] r (:199-200)
__global__ __launch_bounds__(256) void nd_p_kernel(const MshiftState *st, v2d *const *tab, const v2d *r_up, const v2d *r_dn, int ns, int N) {
  const int s = blockIdx.y;
  if (st->done || s >= st->active) return;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N) return;
  const double be = st->betas[s], ze = s ? st->zita[s] : 1.0;
  v2d *pu = tab[4 * s + 2], *pd = tab[4 * s + 3];
#pragma unroll 4
  for (int c = 0; c < 12; c++) {
    const size_t o = (size_t)c * ns + i;
    if (s == 0) { pu[o] = be * pu[o] + r_up[o]; pd[o] = be * pd[o] + r_dn[o]; }
    else { pu[o] = be * pu[o] + ze * r_up[o]; pd[o] = be * pd[o] + ze * r_dn[o]; }
  }
}
}  // namespace

// ---------------------------------------------------------------- host side
struct TmhipNd {
  tmhip_field *s[6];           // operator scratch: [0, 1] EE outputs, [2, 3] first OO output of Qtm_pm_ndpsi, [4, 5] single-flavour hops (two-stencil form)
  tmhip_field *w[6];           // solver: r_up, r_dn, p_up, p_dn, Ap_up, Ap_dn
  tmhip_field *ps[2 * MSHIFT_MAX_SHIFTS];   // shifted directions (allocated as needed)
  int nps;
  double *partials; int max_partials;   // [3][max_partials]: pro, |r|^2, |ps|^2
  MshiftState *st;
  v2d **tab;
};

void tmhip_nd_destroy(tmhip_ctx *ctx) {
  TmhipNd *n = (TmhipNd *)ctx->nd;
  if (!n) return;
  for (int k = 0; k < 6; k++) { tmhip_field_free(ctx, n->s[k]); tmhip_field_free(ctx, n->w[k]); }
  for (int k = 0; k < n->nps; k++) tmhip_field_free(ctx, n->ps[k]);
  if (n->partials) (void)hipFree(n->partials);
  if (n->st) (void)hipFree(n->st);
  if (n->tab) (void)hipFree(n->tab);
  delete n;
  ctx->nd = nullptr;
}

static int nd_prepare(tmhip_ctx *ctx, const char *who) {
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("%s: the doublet operators and solvers run on unsplit lattices only (nproc_t = %d)", who, ctx->g.nproc_t);
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (ctx->nd) return 0;
  TmhipNd *n = new TmhipNd();
  ctx->nd = n;
  for (int k = 0; k < 6; k++)
    if (tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &n->s[k]) || tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &n->w[k])) return 1;
  // stencil: one partial per wave of the padded grid (64-thread blocks, rounded up to a multiple of 8); mix / x kernels: 4 per block
  n->max_partials = ctx->Vh / 64 + 64;
  TMHIP_CHECK(hipMalloc((void **)&n->partials, (size_t)3 * n->max_partials * sizeof(double)));
  TMHIP_CHECK(hipMalloc((void **)&n->st, sizeof(MshiftState)));
  TMHIP_CHECK(hipMalloc((void **)&n->tab, (size_t)4 * MSHIFT_MAX_SHIFTS * sizeof(v2d *)));
  return 0;
}

static bool nd_eo(const tmhip_field *f) { return f && f->kind == TMHIP_FIELD_EO && f->prec == 0; }

static void nd_fill(NdArgs &a, tmhip_ctx *ctx, int ieo) {
  memset(&a, 0, sizeof(a));
  a.gauge = ctx->gauge + (size_t)(ieo ? 1 : 0) * 72 * ctx->gs;
  a.ns = ctx->ns; a.gs = ctx->gs;
  a.T = ctx->g.T; a.LX = ctx->g.LX; a.LY = ctx->g.LY; a.LZh = ctx->g.LZ / 2;
  a.Vh = ctx->Vh; a.face = ctx->face; a.YZh = ctx->g.LY * ctx->g.LZ / 2;
  a.par_off = ieo & 1;
  for (int m = 0; m < 4; m++) { a.ka[m][0] = ctx->ka[m][0]; a.ka[m][1] = ctx->ka[m][1]; }
  a.scale = 1.0;
}

template <int EPI, int BS>
static void nd_launch_hop(tmhip_ctx *ctx, NdArgs a, int *npart) {
  const int nb = ndc::nd_grid(ctx, BS, &a.map_nb, &a.nxcd_chunk);
  const bool cached = ndc::nd_gauge_cached(ctx, sizeof(v2d));
  if constexpr (EPI >= NDSW_EE) {
    if (cached) hipLaunchKernelGGL((ndsw_hop_kernel<EPI, BS, false>), dim3(nb), dim3(BS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((ndsw_hop_kernel<EPI, BS, true>), dim3(nb), dim3(BS), 0, ctx->stream, a);
  } else {
    if (cached) hipLaunchKernelGGL((nd_hop_kernel<EPI, BS, false>), dim3(nb), dim3(BS), 0, ctx->stream, a);
    else hipLaunchKernelGGL((nd_hop_kernel<EPI, BS, true>), dim3(nb), dim3(BS), 0, ctx->stream, a);
  }
  if (npart) *npart = nb * (BS / 64);
}

template <int EPI>
static void nd_launch_mix(tmhip_ctx *ctx, const NdArgs &a, int N, int *npart) {
  const int nb = (N + 255) / 256;
  if constexpr (EPI >= NDSW_EE) hipLaunchKernelGGL((ndsw_mix_kernel<EPI>), dim3(nb), dim3(256), 0, ctx->stream, a, N);
  else hipLaunchKernelGGL((nd_mix_kernel<EPI>), dim3(nb), dim3(256), 0, ctx->stream, a, N);
  if (npart) *npart = 4 * nb;
}

// One hop of a doublet + its mixing epilogue.  out = (out_s, out_c); the accumulators a / b gather in_a / in_b of the other parity.
// ND_EE_INV: mix(a, b; mu, eps) * nrm.  ND_OO[_DOT]: scale * [mix(k_s, k_c; mu, eps) -/+ (a, b)] (+ sigma p, partials of <p, out>).
static int nd_stage(tmhip_ctx *ctx, int epi, int ieo, v2d *out_s, v2d *out_c, const v2d *in_a, const v2d *in_b, const v2d *k_s,
                    const v2d *k_c, double mu, double eps, double scale, const v2d *p_s = nullptr, const v2d *p_c = nullptr,
                    double sigma = 0.0, int *npart = nullptr, double cz_re = 0.0, double cz_im = 0.0) {
  TmhipNd *n = (TmhipNd *)ctx->nd;
  NdArgs a;
  nd_fill(a, ctx, ieo);
  a.cz[0] = cz_re; a.cz[1] = cz_im;
  a.out_s = out_s; a.out_c = out_c; a.k_s = k_s; a.k_c = k_c; a.p_s = p_s; a.p_c = p_c;
  a.mu = mu; a.eps = eps; a.nrm = 1. / (1. + mu * mu - eps * eps); a.scale = scale; a.sigma = sigma;
  a.partials = n->partials;
  if (epi >= NDSW_EE) { a.sw = ctx->sw + (size_t)(ieo ? 1 : 0) * 54 * ctx->gs; a.swi = ctx->sw_inv_nd; }
  if (ctx->opt_nd_fused) {
    a.in_a = in_a; a.in_b = in_b;
    const bool b64 = tmhip_hop_block(ctx) == 64;
    if (b64 && ctx->Vh / 64 + 8 > n->max_partials) TMHIP_FAIL("nd: partials buffer too small");
#define ND_HOP(E) (b64 ? nd_launch_hop<E, 64>(ctx, a, npart) : nd_launch_hop<E, 256>(ctx, a, npart))
    if (epi == ND_EE_INV) ND_HOP(ND_EE_INV);
    else if (epi == ND_OO) ND_HOP(ND_OO);
    else if (epi == ND_OO_SUBC) ND_HOP(ND_OO_SUBC);
    else if (epi == ND_OO_DOT) ND_HOP(ND_OO_DOT);
    else if (epi == NDSW_EE) ND_HOP(NDSW_EE);
    else if (epi == NDSW_OO) ND_HOP(NDSW_OO);
    else if (epi == NDSW_OO_SUBC) ND_HOP(NDSW_OO_SUBC);
    else ND_HOP(NDSW_OO_DOT);
#undef ND_HOP
  } else {
    v2d *ha = n->s[4]->d, *hb = n->s[5]->d;
    if (tmhip_launch_hopping(ctx, ieo, ha, in_a, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    if (tmhip_launch_hopping(ctx, ieo, hb, in_b, nullptr, EPI_STORE, 0, 0, HOP_COMM)) return 1;
    a.in_a = ha; a.in_b = hb;
    if (epi == ND_EE_INV) nd_launch_mix<ND_EE_INV>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO) nd_launch_mix<ND_OO>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO_SUBC) nd_launch_mix<ND_OO_SUBC>(ctx, a, ctx->Vh, npart);
    else if (epi == ND_OO_DOT) nd_launch_mix<ND_OO_DOT>(ctx, a, ctx->Vh, npart);
    else if (epi == NDSW_EE) nd_launch_mix<NDSW_EE>(ctx, a, ctx->Vh, npart);
    else if (epi == NDSW_OO) nd_launch_mix<NDSW_OO>(ctx, a, ctx->Vh, npart);
    else if (epi == NDSW_OO_SUBC) nd_launch_mix<NDSW_OO_SUBC>(ctx, a, ctx->Vh, npart);
    else nd_launch_mix<NDSW_OO_DOT>(ctx, a, ctx->Vh, npart);
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// Qtm_pm_ndpsi (tm_operators_nd.c:195-238): four stages.  l may alias k (the reference allows it): k is last read in stage 2.
static int nd_qpm(tmhip_ctx *ctx, v2d *l_s, v2d *l_c, const v2d *k_s, const v2d *k_c, double scale2,
                  const v2d *p_s = nullptr, const v2d *p_c = nullptr, double sigma = 0.0, int *npart = nullptr) {
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d0 = n->s[0]->d, *d1 = n->s[1]->d, *e0 = n->s[2]->d, *e1 = n->s[3]->d;
  // M_ee_inv(D2, D3; H k_c, H k_s; mubar, eps)                         -- k_charm feeds the first EO hop
  if (nd_stage(ctx, ND_EE_INV, TMHIP_EO, d0, d1, k_c, k_s, nullptr, nullptr, mb, eb, 1.0)) return 1;
  // M_oo_sub_g5(D2', D3'; k_c, k_s; H D2, H D3; -mubar, -eps)
  if (nd_stage(ctx, ND_OO, TMHIP_OE, e0, e1, d0, d1, k_c, k_s, -mb, -eb, 1.0)) return 1;
  // M_ee_inv(D5, D4; H D2', H D3'; -mubar, eps)
  if (nd_stage(ctx, ND_EE_INV, TMHIP_EO, d1, d0, e0, e1, nullptr, nullptr, -mb, eb, 1.0)) return 1;
  // l = invmaxev^2 M_oo_sub_g5(D3', D2'; H D4, H D5; -mubar, -eps)
  return nd_stage(ctx, p_s ? ND_OO_DOT : ND_OO, TMHIP_OE, l_s, l_c, d0, d1, e1, e0, -mb, -eb, scale2, p_s, p_c, sigma, npart);
}

// Qsw_pm_ndpsi (tm_operators_nd.c:240-285): four stages, the clover twins of nd_qpm's.  l may alias k: k is last read in stage 2.
static int ndsw_qpm(tmhip_ctx *ctx, v2d *l_s, v2d *l_c, const v2d *k_s, const v2d *k_c, double scale2,
                    const v2d *p_s = nullptr, const v2d *p_c = nullptr, double sigma = 0.0, int *npart = nullptr) {
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d2 = n->s[0]->d, *d3 = n->s[1]->d, *e3 = n->s[2]->d, *e2 = n->s[3]->d;
  // (D2, D3) = clover_inv_nd assign_mul_one_sw_pm_imu_eps(H k_c, H k_s; -mubar, eps)                        (:245-250)
  if (nd_stage(ctx, NDSW_EE, TMHIP_EO, d2, d3, k_c, k_s, nullptr, nullptr, -mb, eb, 1.0)) return 1;
  // clover_gamma5_nd(l_c = D2', l_s = D3'; k_charm, k_strange; j_c = H D2, j_s = H D3; -mubar, -eps)           (:252-259)
  if (nd_stage(ctx, NDSW_OO, TMHIP_OE, e3, e2, d3, d2, k_s, k_c, -mb, -eb, 1.0)) return 1;
  // (k_s = D7, k_c = D6) from (l_s = H D2', l_c = H D3'; mubar, eps), inverted                                (:265-270); D7 -> d3, D6 -> d2
  if (nd_stage(ctx, NDSW_EE, TMHIP_EO, d3, d2, e2, e3, nullptr, nullptr, mb, eb, 1.0)) return 1;
  // l = invmaxev^2 clover_gamma5_nd(l_charm, l_strange; k_c = D2', k_s = D3'; j_c = H D7, j_s = H D6; mubar, -eps)   (:272-283)
  return nd_stage(ctx, p_s ? NDSW_OO_DOT : NDSW_OO, TMHIP_OE, l_s, l_c, d2, d3, e3, e2, mb, -eb, scale2, p_s, p_c, sigma, npart);
}
// the operator of the solvers: op = TMHIP_ND_OP_QTM_PM | TMHIP_ND_OP_QSW_PM
static int nd_apply_pm(tmhip_ctx *ctx, int op, v2d *l_s, v2d *l_c, const v2d *k_s, const v2d *k_c, double scale2,
                       const v2d *p_s = nullptr, const v2d *p_c = nullptr, double sigma = 0.0, int *npart = nullptr) {
  return op == TMHIP_ND_OP_QSW_PM ? ndsw_qpm(ctx, l_s, l_c, k_s, k_c, scale2, p_s, p_c, sigma, npart)
                                  : nd_qpm(ctx, l_s, l_c, k_s, k_c, scale2, p_s, p_c, sigma, npart);
}

static int nd_check4(tmhip_ctx *ctx, const char *who, tmhip_field *a, tmhip_field *b, tmhip_field *c, tmhip_field *d) {
  if (nd_prepare(ctx, who)) return 1;
  if (!nd_eo(a) || !nd_eo(b) || !nd_eo(c) || !nd_eo(d)) TMHIP_FAIL("%s needs four fp64 one-parity (EO) fields", who);
  if (a->d == b->d) TMHIP_FAIL("%s: the two output flavours must be different fields", who);
  return 0;
}

// the clover doublet: unsplit lattices (the loopback rehearsal counts as split), 1+T resident, and -- need_inv -- sw_inv_nd valid
static int ndsw_check4(tmhip_ctx *ctx, const char *who, bool need_inv, tmhip_field *a, tmhip_field *b, tmhip_field *c, tmhip_field *d) {
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: the clover doublet runs on unsplit lattices only (nproc_t = %d%s)", who, ctx->g.nproc_t, ctx->loopback ? ", loopback" : "");
  return tmhip_ndsw_ready(ctx, who, need_inv) || nd_check4(ctx, who, a, b, c, d);
}

// ---------------------------------------------------------------- solver engine
// Solves (A + sigma_s) x_s = Q, A = Qtm_pm_ndpsi (op 0) or Qsw_pm_ndpsi (op 1), for s = 0 .. nsh-1 (cg_mms_tm_nd.c:64-215; nsh = 1, sigma = 0: cg_her_nd.c:57-160).
// x_up / x_dn: nsh solution pairs; her: x holds the start vector on entry.  Returns the iteration count the reference returns.
static int nd_solve(tmhip_ctx *ctx, int op, bool her, tmhip_field **x_up, tmhip_field **x_dn, tmhip_field *q_up, tmhip_field *q_dn,
                    const double *shifts, int nsh, int max_iter, double eps_sq, int rel_prec, int *iters) {
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const int N = ctx->Vh;
  const double s2 = ctx->invmaxev * ctx->invmaxev;
  tmhip_field *r_up = n->w[0], *r_dn = n->w[1], *p_up = n->w[2], *p_dn = n->w[3], *ap_up = n->w[4], *ap_dn = n->w[5];
  for (; n->nps < 2 * (nsh - 1); n->nps++)
    if (tmhip_field_alloc(ctx, TMHIP_FIELD_EO, &n->ps[n->nps])) return 1;
  MshiftState h;
  memset(&h, 0, sizeof(h));
  double qa, qb;
  if (tmhip_square_norm(ctx, q_up, N, 0, &qa) || tmhip_square_norm(ctx, q_dn, N, 0, &qb)) return 1;
  const double squarenorm = qa + qb;
  if (her) {
    double pa, pb;
    if (tmhip_square_norm(ctx, x_up[0], N, 0, &pa) || tmhip_square_norm(ctx, x_dn[0], N, 0, &pb)) return 1;
    if (pa + pb == 0) {   // cg_her_nd.c:83-91
      if (tmhip_assign(ctx, r_up, q_up, N) || tmhip_assign(ctx, r_dn, q_dn, N)) return 1;
      h.normsq = squarenorm;
    } else {              // :93-104
      if (nd_apply_pm(ctx, op, ap_up->d, ap_dn->d, x_up[0]->d, x_dn[0]->d, s2)) return 1;
      if (tmhip_diff(ctx, r_up, q_up, ap_up, N) || tmhip_diff(ctx, r_dn, q_dn, ap_dn, N)) return 1;
      if (tmhip_square_norm(ctx, r_up, N, 0, &pa) || tmhip_square_norm(ctx, r_dn, N, 0, &pb)) return 1;
      h.normsq = pa + pb;
    }
    h.target = rel_prec == 0 ? eps_sq : (rel_prec == 1 ? eps_sq * squarenorm : -1.0);   // :108: rel_prec other than 0 / 1 never converges
  } else {
    if (tmhip_assign(ctx, r_up, q_up, N) || tmhip_assign(ctx, r_dn, q_dn, N)) return 1;
    for (int s = 0; s < nsh; s++)
      if (tmhip_field_zero(ctx, x_up[s]) || tmhip_field_zero(ctx, x_dn[s])) return 1;
    h.sigma0 = shifts[0] * shifts[0];
    for (int s = 1; s < nsh; s++) {
      h.sigma[s] = shifts[s] * shifts[s] - h.sigma0;
      h.zita[s] = h.zitam1[s] = h.alphas[s] = 1.0;
      if (tmhip_assign(ctx, n->ps[2 * s - 2], q_up, N) || tmhip_assign(ctx, n->ps[2 * s - 1], q_dn, N)) return 1;
    }
    h.normsq = squarenorm;
    h.target = rel_prec > 0 ? eps_sq * squarenorm : (rel_prec == 0 ? eps_sq : -1.0);   // :186-188: rel_prec < 0 runs to max_iter
  }
  if (tmhip_assign(ctx, p_up, r_up, N) || tmhip_assign(ctx, p_dn, r_dn, N)) return 1;
  h.alpha0 = h.alphas[0] = 1.0; h.betas[0] = 0.0;
  h.eps_sq = eps_sq; h.active = h.pact = nsh; h.max_iter = max_iter; h.done_it = -1;
  v2d *tab[4 * MSHIFT_MAX_SHIFTS];
  tab[0] = x_up[0]->d; tab[1] = x_dn[0]->d; tab[2] = p_up->d; tab[3] = p_dn->d;
  for (int s = 1; s < nsh; s++) { tab[4 * s] = x_up[s]->d; tab[4 * s + 1] = x_dn[s]->d; tab[4 * s + 2] = n->ps[2 * s - 2]->d; tab[4 * s + 3] = n->ps[2 * s - 1]->d; }
  TMHIP_CHECK(hipMemcpyAsync(n->tab, tab, sizeof(v2d *) * 4 * nsh, hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(n->st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  const int nbl = (N + 255) / 256;
  double *pa = n->partials, *pr = n->partials + n->max_partials, *psn = n->partials + 2 * n->max_partials;
  if (4 * nbl > n->max_partials) TMHIP_FAIL("nd: partials buffer too small");
  const int batch = ctx->opt_cg_batch > 0 ? ctx->opt_cg_batch : 4;
  if (tmhip_poll_loop(ctx, max_iter, true, batch, 1.0e3 * (h.target > 0 ? h.target : eps_sq), &n->st->done, &n->st->err, 0, false, [&](int iteration) {
        const int check = !her && nsh > 1 && iteration > 0 && iteration % 20 == 0;
        int np = 0;
        if (nd_apply_pm(ctx, op, ap_up->d, ap_dn->d, p_up->d, p_dn->d, s2, p_up->d, p_dn->d, h.sigma0, &np)) return 1;
        hipLaunchKernelGGL(nd_alpha_kernel, dim3(1), dim3(256), 0, ctx->stream, n->st, (const double *)pa, np);
        hipLaunchKernelGGL(nd_x_kernel, dim3(nbl, nsh), dim3(256), 0, ctx->stream, n->st, (v2d *const *)n->tab, r_up->d, r_dn->d,
                           (const v2d *)ap_up->d, (const v2d *)ap_dn->d, ctx->ns, N, pr, psn, check);
        hipLaunchKernelGGL(nd_beta_kernel, dim3(1), dim3(256), 0, ctx->stream, n->st, (const double *)pr, (const double *)psn, 4 * nbl, check, iteration);
        hipLaunchKernelGGL(nd_p_kernel, dim3(nbl, nsh), dim3(256), 0, ctx->stream, (const MshiftState *)n->st, (v2d *const *)n->tab,
                           (const v2d *)r_up->d, (const v2d *)r_dn->d, ctx->ns, N);
        return 0;
      })) return 1;
  TMHIP_CHECK(hipMemcpyAsync(&h, n->st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->nd_active_shifts = h.active;
  if (her) *iters = h.conv ? h.it : -1;                 // cg_her_nd.c:115,159
  else *iters = h.it >= max_iter ? -1 : h.it;           // cg_mms_tm_nd.c:208-209
  return 0;
}

extern "C" {

int tmhip_set_nd(tmhip_ctx *ctx, double mubar, double epsbar, double invmaxev) {
  ctx->mubar = mubar; ctx->epsbar = epsbar; ctx->invmaxev = invmaxev;
  return 0;
}

int tmhip_M_ee_inv_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double mu, double eps) {
  if (nd_check4(ctx, "M_ee_inv_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  NdArgs a;
  nd_fill(a, ctx, 0);
  a.out_s = l_s->d; a.out_c = l_c->d; a.in_a = k_s->d; a.in_b = k_c->d;
  a.mu = mu; a.eps = eps; a.nrm = 1. / (1. + mu * mu - eps * eps);
  nd_launch_mix<ND_EE_INV>(ctx, a, ctx->Vh, nullptr);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_M_oo_sub_g5_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *j_s,
                            tmhip_field *j_c, double mu, double eps) {
  if (nd_check4(ctx, "M_oo_sub_g5_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  if (!nd_eo(j_s) || !nd_eo(j_c)) TMHIP_FAIL("M_oo_sub_g5_ndpsi needs fp64 one-parity (EO) fields");
  NdArgs a;
  nd_fill(a, ctx, 0);
  a.out_s = l_s->d; a.out_c = l_c->d; a.in_a = j_s->d; a.in_b = j_c->d; a.k_s = k_s->d; a.k_c = k_c->d;
  a.mu = mu; a.eps = eps;
  nd_launch_mix<ND_OO>(ctx, a, ctx->Vh, nullptr);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_Qtm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (nd_check4(ctx, "Qtm_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d0 = n->s[0]->d, *d1 = n->s[1]->d;
  // M_ee_inv(D3, D2; H k_s, H k_c; mubar, eps) ; l = invmaxev M_oo_sub_g5(k_s, k_c; H D3, H D2; -mubar, -eps)   (:68-89)
  if (nd_stage(ctx, ND_EE_INV, TMHIP_EO, d1, d0, k_s->d, k_c->d, nullptr, nullptr, mb, eb, 1.0)) return 1;
  return nd_stage(ctx, ND_OO, TMHIP_OE, l_s->d, l_c->d, d1, d0, k_s->d, k_c->d, -mb, -eb, ctx->invmaxev);
}

int tmhip_Qtm_dagger_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (nd_check4(ctx, "Qtm_dagger_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d0 = n->s[0]->d, *d1 = n->s[1]->d;
  // M_ee_inv(D2, D3; H k_c, H k_s; mubar, eps) ; l = invmaxev M_oo_sub_g5(k_s, k_c; j = (H D3, H D2); mubar, -eps)   (:130-152)
  if (nd_stage(ctx, ND_EE_INV, TMHIP_EO, d0, d1, k_c->d, k_s->d, nullptr, nullptr, mb, eb, 1.0)) return 1;
  return nd_stage(ctx, ND_OO, TMHIP_OE, l_s->d, l_c->d, d1, d0, k_s->d, k_c->d, mb, -eb, ctx->invmaxev);
}

/* Q_tau1_sub_const_ndpsi (tm_operators_nd.c:311-380): l = Cpol invev Qhat tau^1 k - Cpol z k.  Two stencil launches; the scaling and the
 * subtraction of the constant are the epilogue of the second.  l must not be k (the reference hops into l before it reads k). */
int tmhip_Q_tau1_sub_const_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double z_re, double z_im,
                                 double Cpol, double invev) {
  if (nd_check4(ctx, "Q_tau1_sub_const_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  if (ctx->loopback) TMHIP_FAIL("Q_tau1_sub_const_ndpsi: unsplit lattices only (loopback)");
  if (l_s->d == k_s->d || l_s->d == k_c->d || l_c->d == k_s->d || l_c->d == k_c->d) TMHIP_FAIL("Q_tau1_sub_const_ndpsi: l must not be k");
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d0 = n->s[0]->d, *d1 = n->s[1]->d;
  // M_ee_inv(D3, D2; H k_c, H k_s; mubar, eps)   (:323-328)
  if (nd_stage(ctx, ND_EE_INV, TMHIP_EO, d1, d0, k_c->d, k_s->d, nullptr, nullptr, mb, eb, 1.0)) return 1;
  // l = Cpol invev M_oo_sub_g5(k_c, k_s; j = (H D3, H D2); -mubar, -eps) - Cpol z (k_s, k_c)   (:330-374)
  return nd_stage(ctx, ND_OO_SUBC, TMHIP_OE, l_s->d, l_c->d, d1, d0, k_c->d, k_s->d, -mb, -eb, Cpol * invev, nullptr, nullptr, 0.0, nullptr,
                  Cpol * z_re, Cpol * z_im);
}

int tmhip_Qtm_pm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (nd_check4(ctx, "Qtm_pm_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  return nd_qpm(ctx, l_s->d, l_c->d, k_s->d, k_c->d, ctx->invmaxev * ctx->invmaxev);
}

int tmhip_H_eo_tm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, int ieo) {
  if (nd_check4(ctx, "H_eo_tm_ndpsi", l_s, l_c, k_s, k_c)) return 1;
  TmhipNd *n = (TmhipNd *)ctx->nd;
  // M_ee_inv(l_c, l_s; H k_s, H k_c; -mubar, eps)   (:508-519): the result lands as (l_charm, l_strange)
  const bool alias = l_s->d == k_s->d || l_s->d == k_c->d || l_c->d == k_s->d || l_c->d == k_c->d;
  v2d *o_c = alias ? n->s[0]->d : l_c->d, *o_s = alias ? n->s[1]->d : l_s->d;
  if (nd_stage(ctx, ND_EE_INV, ieo, o_c, o_s, k_s->d, k_c->d, nullptr, nullptr, -ctx->mubar, ctx->epsbar, 1.0)) return 1;
  if (alias) {   // the reference hops into scratch first, so l may be k
    TMHIP_CHECK(hipMemcpyAsync(l_c->d, o_c, (size_t)12 * ctx->ns * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
    TMHIP_CHECK(hipMemcpyAsync(l_s->d, o_s, (size_t)12 * ctx->ns * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return 0;
}

static int nd_op_check4(tmhip_ctx *ctx, const char *who, int op, tmhip_field *a, tmhip_field *b, tmhip_field *c, tmhip_field *d) {
  if (tmhip_nd_op_check(ctx, who, op)) return 1;
  return tmhip_nd_op_row_of(op)->clover ? ndsw_check4(ctx, who, true, a, b, c, d) : nd_check4(ctx, who, a, b, c, d);
}

int tmhip_cg_her_nd_op(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                       int rel_prec, int N, int op, int *iters) {
  if (nd_op_check4(ctx, "cg_her_nd", op, P_up, P_dn, Q_up, Q_dn)) return 1;
  if (N != ctx->Vh) TMHIP_FAIL("cg_her_nd: N must be VOLUME/2");
  if (max_iter < 0) TMHIP_FAIL("cg_her_nd: max_iter < 0");
  if (max_iter == 0) { *iters = -1; return 0; }
  return nd_solve(ctx, op, true, &P_up, &P_dn, Q_up, Q_dn, nullptr, 1, max_iter, eps_sq, rel_prec, iters);
}

int tmhip_cg_her_nd(tmhip_ctx *ctx, tmhip_field *P_up, tmhip_field *P_dn, tmhip_field *Q_up, tmhip_field *Q_dn, int max_iter, double eps_sq,
                    int rel_prec, int N, int *iters) {
  return tmhip_cg_her_nd_op(ctx, P_up, P_dn, Q_up, Q_dn, max_iter, eps_sq, rel_prec, N, TMHIP_ND_OP_QTM_PM, iters);
}

int tmhip_cg_mms_tm_nd_op(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts,
                          int nshifts, int max_iter, double eps_sq, int rel_prec, int op, int *iters) {
  if (nshifts < 1 || nshifts > MSHIFT_MAX_SHIFTS) TMHIP_FAIL("cg_mms_tm_nd: nshifts = %d is outside [1, %d]", nshifts, MSHIFT_MAX_SHIFTS);
  if (!Pup || !Pdn || !shifts) TMHIP_FAIL("cg_mms_tm_nd: null argument");
  if (nd_op_check4(ctx, "cg_mms_tm_nd", op, Pup[0], Pdn[0], Qup, Qdn)) return 1;
  for (int s = 0; s < nshifts; s++) {
    if (!nd_eo(Pup[s]) || !nd_eo(Pdn[s])) TMHIP_FAIL("cg_mms_tm_nd needs fp64 one-parity (EO) solution fields");
    if (Pup[s]->d == Qup->d || Pup[s]->d == Qdn->d || Pdn[s]->d == Qup->d || Pdn[s]->d == Qdn->d) TMHIP_FAIL("cg_mms_tm_nd: a solution field is the source");
  }
  if (max_iter < 1) TMHIP_FAIL("cg_mms_tm_nd: max_iter < 1");
  return nd_solve(ctx, op, false, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, iters);
}

int tmhip_cg_mms_tm_nd(tmhip_ctx *ctx, tmhip_field **Pup, tmhip_field **Pdn, tmhip_field *Qup, tmhip_field *Qdn, const double *shifts,
                       int nshifts, int max_iter, double eps_sq, int rel_prec, int *iters) {
  return tmhip_cg_mms_tm_nd_op(ctx, Pup, Pdn, Qup, Qdn, shifts, nshifts, max_iter, eps_sq, rel_prec, TMHIP_ND_OP_QTM_PM, iters);
}

/* ---- the clover doublet (operator/tm_operators_nd.c, operator/clovertm_operators.c); "_s" = strange = up, "_c" = charm = dn ---- */
static int ndsw_local(tmhip_ctx *ctx, int epi, int ieo, v2d *out_s, v2d *out_c, const v2d *in_s, const v2d *in_c, const v2d *k_s, const v2d *k_c,
                      double mu, double eps) {
  NdArgs a;
  nd_fill(a, ctx, ieo);
  a.out_s = out_s; a.out_c = out_c; a.in_a = in_s; a.in_b = in_c; a.k_s = k_s; a.k_c = k_c;
  a.mu = mu; a.eps = eps;
  a.sw = ctx->sw + (size_t)(ieo ? 1 : 0) * 54 * ctx->gs; a.swi = ctx->sw_inv_nd;
  if (epi == NDSW_MUL) nd_launch_mix<NDSW_MUL>(ctx, a, ctx->Vh, nullptr);
  else if (epi == NDSW_INV) nd_launch_mix<NDSW_INV>(ctx, a, ctx->Vh, nullptr);
  else if (epi == NDSW_EE) nd_launch_mix<NDSW_EE>(ctx, a, ctx->Vh, nullptr);
  else nd_launch_mix<NDSW_OO>(ctx, a, ctx->Vh, nullptr);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

/* assign_mul_one_sw_pm_imu_eps(ieo, k_s, k_c, l_s, l_c, mu, eps)   clovertm_operators.c:960-1074; k may be l */
int tmhip_assign_mul_one_sw_pm_imu_eps(tmhip_ctx *ctx, int ieo, tmhip_field *k_s, tmhip_field *k_c, tmhip_field *l_s, tmhip_field *l_c, double mu,
                                       double eps) {
  if (ndsw_check4(ctx, "assign_mul_one_sw_pm_imu_eps", false, k_s, k_c, l_s, l_c)) return 1;
  return ndsw_local(ctx, NDSW_MUL, ieo, k_s->d, k_c->d, l_s->d, l_c->d, nullptr, nullptr, mu, eps);
}

/* clover_inv_nd(ieo, l_c, l_s)   clovertm_operators.c:352-425, in place; sw_inv_nd belongs to the even sites: ieo = EE only */
int tmhip_clover_inv_nd(tmhip_ctx *ctx, int ieo, tmhip_field *l_c, tmhip_field *l_s) {
  if (ieo != 0) TMHIP_FAIL("clover_inv_nd: sw_invert_nd inverts the even sites only (ieo = %d)", ieo);
  if (ndsw_check4(ctx, "clover_inv_nd", true, l_s, l_c, l_s, l_c)) return 1;
  return ndsw_local(ctx, NDSW_INV, 0, l_s->d, l_c->d, l_s->d, l_c->d, nullptr, nullptr, 0.0, 0.0);
}

/* clover_gamma5_nd(ieo, l_c, l_s, k_c, k_s, j_c, j_s, mubar, epsbar)   clovertm_operators.c:733-850; l may be k or j */
int tmhip_clover_gamma5_nd(tmhip_ctx *ctx, int ieo, tmhip_field *l_c, tmhip_field *l_s, tmhip_field *k_c, tmhip_field *k_s, tmhip_field *j_c,
                           tmhip_field *j_s, double mubar, double epsbar) {
  if (ndsw_check4(ctx, "clover_gamma5_nd", false, l_s, l_c, k_s, k_c)) return 1;
  if (!nd_eo(j_s) || !nd_eo(j_c)) TMHIP_FAIL("clover_gamma5_nd needs fp64 one-parity (EO) fields");
  return ndsw_local(ctx, NDSW_OO, ieo, l_s->d, l_c->d, j_s->d, j_c->d, k_s->d, k_c->d, mubar, epsbar);
}

/* Qsw_ndpsi (tm_operators_nd.c:91-111) and Qsw_dagger_ndpsi (:154-174): the same two stages at +mubar / -mubar */
static int ndsw_q(tmhip_ctx *ctx, const char *who, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double mb) {
  if (ndsw_check4(ctx, who, true, l_s, l_c, k_s, k_c)) return 1;
  TmhipNd *n = (TmhipNd *)ctx->nd;
  v2d *d2 = n->s[0]->d, *d3 = n->s[1]->d;
  // (k_s = D2, k_c = D3) from (l_s = H k_c, l_c = H k_s; mb, eps), inverted ; clover_gamma5_nd(D2', D3'; k_charm, k_strange; j_c = H D2, j_s = H D3; mb, -eps)
  if (nd_stage(ctx, NDSW_EE, TMHIP_EO, d2, d3, k_c->d, k_s->d, nullptr, nullptr, mb, ctx->epsbar, 1.0)) return 1;
  return nd_stage(ctx, NDSW_OO, TMHIP_OE, l_s->d, l_c->d, d3, d2, k_s->d, k_c->d, mb, -ctx->epsbar, ctx->invmaxev);
}
int tmhip_Qsw_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  return ndsw_q(ctx, "Qsw_ndpsi", l_s, l_c, k_s, k_c, ctx->mubar);
}
int tmhip_Qsw_dagger_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  return ndsw_q(ctx, "Qsw_dagger_ndpsi", l_s, l_c, k_s, k_c, -ctx->mubar);
}

/* Qsw_pm_ndpsi (:240-285); l may be k */
int tmhip_Qsw_pm_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (ndsw_check4(ctx, "Qsw_pm_ndpsi", true, l_s, l_c, k_s, k_c)) return 1;
  return ndsw_qpm(ctx, l_s->d, l_c->d, k_s->d, k_c->d, ctx->invmaxev * ctx->invmaxev);
}

/* Qsw_tau1_sub_const_ndpsi (:378-444): two stencil launches, the scaling and the subtracted constant in the epilogue of the second.
 * The reference's statements are followed literally: its assign_mul_one_sw_pm_imu_eps writes (k_s, k_c) = (D3, D2) (:393-394), so
 * clover_gamma5_nd's "_s" output, built on k_strange, ends as l_charm.  l must not be k. */
int tmhip_Qsw_tau1_sub_const_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c, double z_re, double z_im,
                                   double Cpol, double invev) {
  if (ndsw_check4(ctx, "Qsw_tau1_sub_const_ndpsi", true, l_s, l_c, k_s, k_c)) return 1;
  if (l_s->d == k_s->d || l_s->d == k_c->d || l_c->d == k_s->d || l_c->d == k_c->d) TMHIP_FAIL("Qsw_tau1_sub_const_ndpsi: l must not be k");
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const double mb = ctx->mubar, eb = ctx->epsbar;
  v2d *d3 = n->s[0]->d, *d2 = n->s[1]->d;
  // (k_s = D3, k_c = D2) from (l_s = H k_c, l_c = H k_s; -mubar, eps), inverted   (:390-395)
  if (nd_stage(ctx, NDSW_EE, TMHIP_EO, d3, d2, k_c->d, k_s->d, nullptr, nullptr, -mb, eb, 1.0)) return 1;
  // clover_gamma5_nd(l_c = D0, l_s = D1; k_charm, k_strange; j_c = H D3, j_s = H D2; -mubar, -eps); l_strange = Cpol invev D0 - Cpol z k_strange,
  // l_charm = Cpol invev D1 - Cpol z k_charm   (:397-441)
  return nd_stage(ctx, NDSW_OO_SUBC, TMHIP_OE, l_c->d, l_s->d, d2, d3, k_s->d, k_c->d, -mb, -eb, Cpol * invev, nullptr, nullptr, 0.0, nullptr,
                  Cpol * z_re, Cpol * z_im);
}

/* H_eo_sw_ndpsi (:521-535): assign_mul_one_sw_pm_imu_eps(EE, l_charm, l_strange; H k_s, H k_c; mubar, eps), then clover_inv_nd; l may be k */
int tmhip_H_eo_sw_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (ndsw_check4(ctx, "H_eo_sw_ndpsi", true, l_s, l_c, k_s, k_c)) return 1;
  TmhipNd *n = (TmhipNd *)ctx->nd;
  const bool alias = l_s->d == k_s->d || l_s->d == k_c->d || l_c->d == k_s->d || l_c->d == k_c->d;
  v2d *o_c = alias ? n->s[0]->d : l_c->d, *o_s = alias ? n->s[1]->d : l_s->d;
  if (nd_stage(ctx, NDSW_EE, TMHIP_EO, o_c, o_s, k_s->d, k_c->d, nullptr, nullptr, ctx->mubar, ctx->epsbar, 1.0)) return 1;
  if (alias) {   // the reference hops into scratch first
    TMHIP_CHECK(hipMemcpyAsync(l_c->d, o_c, (size_t)12 * ctx->ns * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
    TMHIP_CHECK(hipMemcpyAsync(l_s->d, o_s, (size_t)12 * ctx->ns * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return 0;
}

/* Msw_ee_inv_ndpsi (:539-549): site-local, assign_mul_one_sw_pm_imu_eps(EE, l; k; -mubar, eps) then clover_inv_nd; l may be k */
int tmhip_Msw_ee_inv_ndpsi(tmhip_ctx *ctx, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  if (ndsw_check4(ctx, "Msw_ee_inv_ndpsi", true, l_s, l_c, k_s, k_c)) return 1;
  return ndsw_local(ctx, NDSW_EE, 0, l_s->d, l_c->d, k_s->d, k_c->d, nullptr, nullptr, -ctx->mubar, ctx->epsbar);
}

int tmhip_nd_active_shifts(tmhip_ctx *ctx) { return ctx->nd_active_shifts; }

}  // extern "C"
