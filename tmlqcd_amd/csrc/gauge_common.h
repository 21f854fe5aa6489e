// Device functions shared by the kernels that walk the lexicographic resident links (gauge.hip: gauge monomial; flow.hip: Wilson flow
// and clover field strength): complex 3x3 products, the site geometry with its one-conditional wrap, the path product and the staple sums.
#pragma once
#include "tmhip_internal.h"

namespace gaugehip {
typedef v2d cd;
__device__ __forceinline__ cd g_cmul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd g_cmulc(cd a, cd b) { return cd{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }    // a conj(b)

// u = v w and u = v w^dagger (su3.h:583-626): each element is the sum of three products, left to right
__device__ __forceinline__ void mm(cd (&u)[9], const cd (&v)[9], const cd (&w)[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) u[3 * i + j] = g_cmul(v[3 * i], w[j]) + g_cmul(v[3 * i + 1], w[3 + j]) + g_cmul(v[3 * i + 2], w[6 + j]);
}
__device__ __forceinline__ void mmd(cd (&u)[9], const cd (&v)[9], const cd (&w)[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) u[3 * i + j] = g_cmulc(v[3 * i], w[3 * j]) + g_cmulc(v[3 * i + 1], w[3 * j + 1]) + g_cmulc(v[3 * i + 2], w[3 * j + 2]);
}
// Re tr(v w^dagger), the nine terms in the order of su3.h:656-665
__device__ __forceinline__ double retr_mmd(const cd (&v)[9], const cd (&w)[9]) {
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 9; e++) s += v[e].x * w[e].x + v[e].y * w[e].y;
  return s;
}

struct GaugeGeom {
  int V, Vh, T, LX, LY, LZ, XYZ, toff;
  int slab[4];   // first site of the time-slices t = T, T + 1, -1, -2: periodic images, or the halo slabs of a T-split rank (T, -1 only)
};

// Coordinates of a site plus up to two steps along two directions -> index into the lexicographic field.  Periodic in space (one
// conditional wrap is enough for |step| <= 2 <= extent, extent 2 included where x + 2 == x); a time-slice outside [0, T) is looked up in
// GaugeGeom::slab, so the unsplit lattice and a T-split rank (t = T and t = -1 are the halo slabs behind the VOLUME own sites; callers
// never step further there) share one branch-free form.
struct Site {
  int t, x, y, z;
};
__device__ __forceinline__ Site g_shift(Site s, int dir, int n) {
  s.t += dir == 0 ? n : 0;
  s.x += dir == 1 ? n : 0;
  s.y += dir == 2 ? n : 0;
  s.z += dir == 3 ? n : 0;
  return s;
}
__device__ __forceinline__ int g_wrap(int c, int L) { return c < 0 ? c + L : (c >= L ? c - L : c); }
__device__ __forceinline__ int g_index(const GaugeGeom &g, Site s) {
  const int x = g_wrap(s.x, g.LX), y = g_wrap(s.y, g.LY), z = g_wrap(s.z, g.LZ);
  const int sp = (x * g.LY + y) * g.LZ + z;
  const int above = s.t == g.T ? g.slab[0] : g.slab[1], below = s.t == -1 ? g.slab[2] : g.slab[3];
  const int base = s.t >= g.T ? above : (s.t < 0 ? below : s.t * g.XYZ);
  return base + sp;
}
__device__ __forceinline__ void g_load(cd (&u)[9], const v2d *__restrict__ raw, const GaugeGeom &g, Site s, int mu) {
  const int ix = g_index(g, s);
  const v2d *p = raw + ((size_t)ix * 4 + mu) * 9;
#pragma unroll
  for (int e = 0; e < 9; e++) u[e] = p[e];
}
__device__ __forceinline__ Site g_site(const GaugeGeom &g, int ix) {
  Site s;
  s.z = ix % g.LZ;
  int r = ix / g.LZ;
  s.y = r % g.LY;
  r /= g.LY;
  s.x = r % g.LX;
  s.t = r / g.LX;
  return s;
}

// su3adj.h:164-172: d += c trlambda(w), eight planes Vh doubles apart
__device__ __forceinline__ void g_trace_lambda_add(double *__restrict__ d, size_t st, double c, const cd (&w)[9]) {
  d[0 * st] += c * (-w[3].y - w[1].y);
  d[1 * st] += c * (+w[3].x - w[1].x);
  d[2 * st] += c * (-w[0].y + w[4].y);
  d[3 * st] += c * (-w[6].y - w[2].y);
  d[4 * st] += c * (+w[6].x - w[2].x);
  d[5 * st] += c * (-w[7].y - w[5].y);
  d[6 * st] += c * (+w[7].x - w[5].x);
  d[7 * st] += c * ((-w[0].y - w[4].y + 2.0 * w[8].y) * 0.577350269189625);
}

// A staple is a path of links from x to x + mu.  Step codes: 0 = +nu, 1 = -nu, 2 = +mu, 3 = -mu; a forward step multiplies by the
// link at the current site and moves on, a backward step moves first and multiplies by the adjoint.  A path is its codes packed two
// bits per step.  The product is built left to right with three matrices live (product so far, link, new product); the step loop is
// rolled (the branches in it are wave-uniform), so the whole staple sum is a few hundred instructions of code.
__host__ __device__ constexpr unsigned g_path(int a, int b, int c, int d = 0, int e = 0) {
  return (unsigned)(a | (b << 2) | (c << 4) | (d << 6) | (e << 8));
}
template <int NSTEP>
__device__ __forceinline__ void path_product(cd (&acc)[9], const v2d *__restrict__ raw, const GaugeGeom &g, Site y, int mu, int nu, unsigned code) {
#pragma unroll 1
  for (int j = 0; j < NSTEP; j++) {
    const unsigned c = (code >> (2 * j)) & 3u;
    const int dir = (c & 2u) ? mu : nu;
    const bool back = (c & 1u) != 0;
    if (back) y = g_shift(y, dir, -1);
    cd l[9];
    g_load(l, raw, g, y, dir);
    if (!back) y = g_shift(y, dir, 1);
    if (j == 0) {
      if (back) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int q = 0; q < 3; q++) acc[3 * r + q] = cd{l[3 * q + r].x, -l[3 * q + r].y};
      } else {
#pragma unroll
        for (int e = 0; e < 9; e++) acc[e] = l[e];
      }
    } else {
      cd t[9];
      if (back) mmd(t, acc, l); else mm(t, acc, l);
#pragma unroll
      for (int e = 0; e < 9; e++) acc[e] = t[e];
    }
  }
}

// Plaquette staples of the link (s, mu), get_staples.c:34-69: per k != mu the staple above, then the one below.  Each plane is weighted:
// planes with direction 0 by wt, the purely spatial ones by ws (gauge_EMderivative's 1 + lambda / 1 - lambda; both exactly 1 for
// gauge_derivative).
__device__ __forceinline__ void plaquette_staples(cd (&v)[9], const v2d *__restrict__ raw, const GaugeGeom &g, Site s, int mu, double wt, double ws) {
#pragma unroll
  for (int e = 0; e < 9; e++) v[e] = cd{0.0, 0.0};
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    if (k == mu) continue;
    const double w = (k == 0 || mu == 0) ? wt : ws;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      cd acc[9];
      path_product<3>(acc, raw, g, s, mu, k, h == 0 ? g_path(0, 2, 1) : g_path(1, 2, 0));
#pragma unroll
      for (int e = 0; e < 9; e++) v[e] += cd{w * acc[e].x, w * acc[e].y};
    }
  }
}

// Rectangle staples of the link (s, mu), get_rectangle_staples.c:33-186: six five-link paths per nu != mu, summed in that file's order
// (2 x 1 above, 2 x 1 below, 1 x 2 above and below starting at x, 1 x 2 below and above starting at x - mu).
__device__ __forceinline__ void rectangle_staples(cd (&v)[9], const v2d *__restrict__ raw, const GaugeGeom &g, Site s, int mu) {
#pragma unroll
  for (int e = 0; e < 9; e++) v[e] = cd{0.0, 0.0};
#pragma unroll 1
  for (int nu = 0; nu < 4; nu++) {
    if (nu == mu) continue;
#pragma unroll 1
    for (int h = 0; h < 6; h++) {
      const unsigned code = h == 0 ? g_path(0, 0, 2, 1, 1) : h == 1 ? g_path(1, 1, 2, 0, 0) : h == 2 ? g_path(0, 2, 2, 1, 3)
                          : h == 3 ? g_path(1, 2, 2, 0, 3) : h == 4 ? g_path(3, 1, 2, 2, 0) : g_path(3, 0, 2, 2, 1);
      cd acc[9];
      path_product<5>(acc, raw, g, s, mu, nu, code);
#pragma unroll
      for (int e = 0; e < 9; e++) v[e] += acc[e];
    }
  }
}

// the library's reproducible reduction (linalg.hip): butterfly within the wave, the four wave sums added in order, one partial per block
__device__ __forceinline__ void g_block_reduce_store(double v, double *partials) {
  __shared__ double wsum[4];
  v = tmhip_wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

GaugeGeom gauge_geom(const tmhip_ctx *ctx);
int gauge_ready(tmhip_ctx *ctx, const char *who, bool rectangles);
int gauge_sum(tmhip_ctx *ctx, const v2d *links, bool rectangles, double wt, double ws, double *out);
}  // namespace gaugehip
