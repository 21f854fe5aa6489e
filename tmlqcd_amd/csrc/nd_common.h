// The parts of the doublet stencil that do not depend on the precision, shared by nd.hip (fp64) and nd32.hip (fp32): complex
// arithmetic on v2d / v2f, the spin projection and reconstruction of one hop, and the neighbour indices of a site.
#pragma once
#include "tmhip_internal.h"

namespace ndc {
template <class V> __device__ __forceinline__ V cfma(V a, V b, V c) {   // c + a*b
  const V t = __builtin_elementwise_fma(V{a.x, a.x}, b, c);
  return __builtin_elementwise_fma(V{-a.y, a.y}, V{b.y, b.x}, t);
}
template <class V> __device__ __forceinline__ V cfmac(V a, V b, V c) {  // c + conj(a)*b
  const V t = __builtin_elementwise_fma(V{a.x, a.x}, b, c);
  return __builtin_elementwise_fma(V{a.y, -a.y}, V{b.y, b.x}, t);
}
template <class V> __device__ __forceinline__ V cmul(V a, V b) { return __builtin_elementwise_fma(V{-a.y, a.y}, V{b.y, b.x}, V{a.x, a.x} * b); }
template <class V> __device__ __forceinline__ V cmulc(V a, V b) { return __builtin_elementwise_fma(V{a.y, -a.y}, V{b.y, b.x}, V{a.x, a.x} * b); }

// projection (1 -+ gamma_mu) of one spinor for hop D = 2 mu + (0: +mu, 1: -mu); the same lines as hop_dir (hopping_impl.inc)
template <int D, class V>
__device__ __forceinline__ void nd_project(const V (&s)[12], V (&pa)[3], V (&pb)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const V s0 = s[c], s1 = s[3 + c], s2 = s[6 + c], s3 = s[9 + c];
    if (D == 0) { pa[c] = s0 + s2; pb[c] = s1 + s3; }
    if (D == 1) { pa[c] = s0 - s2; pb[c] = s1 - s3; }
    if (D == 2) { pa[c] = V{s0.x - s3.y, s0.y + s3.x}; pb[c] = V{s1.x - s2.y, s1.y + s2.x}; }
    if (D == 3) { pa[c] = V{s0.x + s3.y, s0.y - s3.x}; pb[c] = V{s1.x + s2.y, s1.y - s2.x}; }
    if (D == 4) { pa[c] = s0 + s3; pb[c] = s1 - s2; }
    if (D == 5) { pa[c] = s0 - s3; pb[c] = s1 + s2; }
    if (D == 6) { pa[c] = V{s0.x - s2.y, s0.y + s2.x}; pb[c] = V{s1.x + s3.y, s1.y - s3.x}; }
    if (D == 7) { pa[c] = V{s0.x + s2.y, s0.y - s2.x}; pb[c] = V{s1.x - s3.y, s1.y + s3.x}; }
  }
}

// link times half-spinor, ka, and the reconstruction into the accumulator
template <int D, class V>
__device__ __forceinline__ void nd_apply(V (&acc)[12], const V (&u)[9], const V (&pa)[3], const V (&pb)[3], V ka) {
  V ca[3], cb[3];
  if ((D & 1) == 0) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      ca[r] = cfma(u[3 * r + 2], pa[2], cfma(u[3 * r + 1], pa[1], cmul(u[3 * r], pa[0])));
      cb[r] = cfma(u[3 * r + 2], pb[2], cfma(u[3 * r + 1], pb[1], cmul(u[3 * r], pb[0])));
    }
#pragma unroll
    for (int r = 0; r < 3; r++) { ca[r] = cmul(ka, ca[r]); cb[r] = cmul(ka, cb[r]); }
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      ca[r] = cfmac(u[6 + r], pa[2], cfmac(u[3 + r], pa[1], cmulc(u[r], pa[0])));
      cb[r] = cfmac(u[6 + r], pb[2], cfmac(u[3 + r], pb[1], cmulc(u[r], pb[0])));
    }
#pragma unroll
    for (int r = 0; r < 3; r++) { ca[r] = cmulc(ka, ca[r]); cb[r] = cmulc(ka, cb[r]); }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const V a = ca[c], b = cb[c];
    acc[c] += a;
    acc[3 + c] += b;
    if (D == 0) { acc[6 + c] += a; acc[9 + c] += b; }
    if (D == 1) { acc[6 + c] -= a; acc[9 + c] -= b; }
    if (D == 2) { acc[9 + c] += V{a.y, -a.x}; acc[6 + c] += V{b.y, -b.x}; }
    if (D == 3) { acc[9 + c] += V{-a.y, a.x}; acc[6 + c] += V{-b.y, b.x}; }
    if (D == 4) { acc[9 + c] += a; acc[6 + c] -= b; }
    if (D == 5) { acc[9 + c] -= a; acc[6 + c] += b; }
    if (D == 6) { acc[6 + c] += V{a.y, -a.x}; acc[9 + c] += V{-b.y, b.x}; }
    if (D == 7) { acc[6 + c] += V{-a.y, a.x}; acc[9 + c] += V{b.y, -b.x}; }
  }
}

// The site-local mixing of the two flavours on the six components of chirality b (0: spins 0, 1; 1: spins 2, 3), in registers:
//   EE  (M_ee_inv_ndpsi):     o = fac [(1 -+ i mu) k_s + eps k_c],  fac [(1 +- i mu) k_c + eps k_s]          fac = nrm
//   !EE (M_oo_sub_g5_ndpsi):  o = fac [that - j] on spins 0, 1 and fac [j - that] on spins 2, 3                fac = the mul_r behind it
// R: the real type of V; mu, eps and fac arrive rounded to it.
template <bool EE, class V, class R>
__device__ __forceinline__ void nd_mix6(int b, R mu, R eps, R fac, const V *ks, const V *kc, const V *js, const V *jc, V *os, V *oc) {
  const V zs = V{(R)1.0, b == 0 ? -mu : mu}, zc = V{(R)1.0, b == 0 ? mu : -mu};
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const V phi1 = cmul(zs, ks[c]) + eps * kc[c];   // _complex_times_vector + _vector_add_mul
    const V phi2 = cmul(zc, kc[c]) + eps * ks[c];
    if (EE) {
      os[c] = fac * phi1; oc[c] = fac * phi2;
    } else {
      os[c] = fac * (b == 0 ? phi1 - js[c] : js[c] - phi1);   // then mul_r(l, phmc_invmaxev, ..)
      oc[c] = fac * (b == 0 ? phi2 - jc[c] : jc[c] - phi2);
    }
  }
}

// the e/o sub-indices of the eight neighbours of output site i, in the order +t, -t, +x, -x, +y, -y, +z, -z.  A: the kernel's argument
// block (T, LX, LY, LZh, face = LX LY LZ / 2, YZh = LY LZ / 2, par_off = parity of the output sites)
template <class A>
__device__ __forceinline__ void nd_neighbours(const A &a, int i, int (&j)[8]) {
  const int LZh = a.LZh;
  const int k = i % LZh;
  int r = i / LZh;
  const int y = r % a.LY;
  r /= a.LY;
  const int x = r % a.LX;
  const int t = r / a.LX;
  const int o = (t + x + y + a.par_off) & 1;   // z = 2k + o  (geometry_eo.c:807-811)
  const int XYZh = a.face, YZh = a.YZh;
  j[0] = (t + 1 < a.T) ? i + XYZh : i - (a.T - 1) * XYZh;
  j[1] = (t > 0) ? i - XYZh : i + (a.T - 1) * XYZh;
  j[2] = (x + 1 < a.LX) ? i + YZh : i - (a.LX - 1) * YZh;
  j[3] = (x > 0) ? i - YZh : i + (a.LX - 1) * YZh;
  j[4] = (y + 1 < a.LY) ? i + LZh : i - (a.LY - 1) * LZh;
  j[5] = (y > 0) ? i - LZh : i + (a.LY - 1) * LZh;
  j[6] = o ? ((k + 1 < LZh) ? i + 1 : i - (LZh - 1)) : i;
  j[7] = o ? i : ((k > 0) ? i - 1 : i + (LZh - 1));
}

// the grid of a doublet stencil launch: nb blocks of BS threads; with "xcd" on and at least 64 blocks the grid is
// padded to a multiple of eight and blocks b, b + 8, .. take one contiguous chunk of the lattice.  Returns the blocks to launch.
static inline int nd_grid(const tmhip_ctx *ctx, int BS, int *map_nb, int *nxcd_chunk) {
  int nb = (ctx->Vh + BS - 1) / BS;
  *map_nb = nb;
  *nxcd_chunk = 0;
  if (ctx->opt_xcd && nb >= 64) { *nxcd_chunk = (nb + 7) / 8; nb = 8 * *nxcd_chunk; }
  return nb;
}
// the links stay in the Infinity Cache between calls while the gauge copy is small (the rule of hop_kernel's GAUX = -2)
static inline bool nd_gauge_cached(const tmhip_ctx *ctx, size_t elem_bytes) {
  return ctx->opt_gauge_cache < 0 ? (size_t)2 * 72 * ctx->gs * elem_bytes <= (size_t)200 << 20 : ctx->opt_gauge_cache != 0;
}
}  // namespace ndc
