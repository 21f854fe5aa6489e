// Gauge monomial (monomial/gauge_monomial.c) on the device-resident links: force and action of the plaquette and the rectangle term.
//   tmhip_gauge_derivative      gauge_derivative / gauge_EMderivative (gauge_monomial.c:48-162): for every link (x, mu)
//                               deriv(x, mu) += factor trlambda( U_mu(x) staple^dagger ), staples as get_staples.c:34-69 and
//                               get_rectangle_staples.c:33-186
//   tmhip_measure_plaquette, tmhip_measure_gauge_action (measure_gauge_action.c:46-189), tmhip_measure_rectangles
//                               (measure_rectangles.c:51-140)
// Layout read: the lexicographic field ctx->gauge_raw ([VPR][4][9] complex, what tmhip_set_gauge received and tmhip_update_gauge
// updates in place).  It is the only copy that holds the halo slabs of a T-split rank (t = T at [V, V + XYZ), t = -1 behind it), a
// neighbour in any direction is one index computation away, and no re-sort stands between an update_gauge and the next force.
// Gather formulation: ONE thread owns a link, adds up all of that link's staples in the reference's order and does the single
// read-modify-write of its eight derivative entries -- no atomics, bit-identical from call to call.
// Block shape: 256 threads = 64 consecutive lexicographic sites (whole z-rows of one (t, x) row for LZ <= 64) x the four directions,
// wave w of the block takes direction mu = w: mu is wave-uniform (no divergence in the "nu != mu" loops) and the four waves together
// walk the block's 64 x 576 contiguous bytes of links, so the staples' re-reads of the block's own and the neighbouring rows are served
// by L2.  The loops over nu, the paths and their steps are rolled: unrolled, the rectangle body alone is 72 matrix products per nu and
// the compiler gathers its 30 link loads in front of them and spills.
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

// deriv[par][mu][8][Vh] += fp trlambda(U staple_plaq^dagger) (+ fr trlambda(U staple_rect^dagger)),  gauge_monomial.c:71-85
template <bool RECT>
__global__ __launch_bounds__(256, 2) void gauge_force_kernel(const v2d *__restrict__ raw, double *__restrict__ deriv, GaugeGeom g, double fp, double fr,
                                                             double wt, double ws) {
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mu = threadIdx.x >> 6;
  if (ix >= g.V) return;
  const Site s = g_site(g, ix);
  const int par = (s.t + s.x + s.y + s.z + g.toff) & 1;
  double *d = deriv + ((size_t)par * 32 + (size_t)mu * 8) * g.Vh + (ix >> 1);
  cd u[9], v[9], w[9];
  plaquette_staples(v, raw, g, s, mu, wt, ws);
  g_load(u, raw, g, s, mu);
  mmd(w, u, v);
  g_trace_lambda_add(d, (size_t)g.Vh, fp, w);
  if (RECT) {
    rectangle_staples(v, raw, g, s, mu);
    g_load(u, raw, g, s, mu);
    mmd(w, u, v);
    g_trace_lambda_add(d, (size_t)g.Vh, fr, w);
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

// sum over the own sites and the six planes mu1 < mu2 of w Re tr( U_mu1(x) U_mu2(x+mu1) [U_mu2(x) U_mu1(x+mu2)]^dagger ), planes with
// direction 0 weighted wt, the others ws (measure_gauge_action.c:129-168; wt = ws = 1: measure_plaquette, :67-86), in that order per site
__global__ __launch_bounds__(256, 2) void plaquette_sum_kernel(const v2d *__restrict__ raw, GaugeGeom g, double wt, double ws, double *partials) {
  const int ix = blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (ix < g.V) {
    const Site s = g_site(g, ix);
#pragma unroll 1
    for (int mu1 = 0; mu1 < 3; mu1++)
#pragma unroll 1
      for (int mu2 = mu1 + 1; mu2 < 4; mu2++) {
        cd a[9], b[9], p1[9], p2[9];
        g_load(a, raw, g, s, mu1);
        g_load(b, raw, g, g_shift(s, mu1, 1), mu2);
        mm(p1, a, b);
        g_load(a, raw, g, s, mu2);
        g_load(b, raw, g, g_shift(s, mu2, 1), mu1);
        mm(p2, a, b);
        acc += (mu1 == 0 ? wt : ws) * retr_mmd(p1, p2);
      }
  }
  g_block_reduce_store(acc, partials);
}

// sum over the own sites and the twelve (mu, nu != mu) of Re tr( U_mu(x) U_nu(x+mu) U_nu(x+mu+nu) [U_nu(x) U_nu(x+nu) U_mu(x+2nu)]^dagger ),
// measure_rectangles.c:73-118
__global__ __launch_bounds__(256, 2) void rectangle_sum_kernel(const v2d *__restrict__ raw, GaugeGeom g, double *partials) {
  const int ix = blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (ix < g.V) {
    const Site s = g_site(g, ix);
#pragma unroll 1
    for (int mu = 0; mu < 4; mu++)
#pragma unroll 1
      for (int nu = 0; nu < 4; nu++) {
        if (nu == mu) continue;
        cd a[9], b[9], tmp[9], p1[9], p2[9];
        const Site j = g_shift(s, mu, 1);
        g_load(a, raw, g, s, mu);
        g_load(b, raw, g, j, nu);
        mm(tmp, a, b);
        g_load(a, raw, g, g_shift(j, nu, 1), nu);
        mm(p1, tmp, a);
        g_load(a, raw, g, s, nu);
        g_load(b, raw, g, g_shift(s, nu, 1), nu);
        mm(tmp, a, b);
        g_load(a, raw, g, g_shift(s, nu, 2), mu);
        mm(p2, tmp, a);
        acc += retr_mmd(p1, p2);
      }
  }
  g_block_reduce_store(acc, partials);
}

GaugeGeom gauge_geom(const tmhip_ctx *ctx) {
  GaugeGeom g;
  g.V = ctx->V; g.Vh = ctx->Vh; g.T = ctx->g.T; g.LX = ctx->g.LX; g.LY = ctx->g.LY; g.LZ = ctx->g.LZ;
  g.XYZ = ctx->g.LX * ctx->g.LY * ctx->g.LZ; g.toff = ctx->g.proc_t * ctx->g.T;
  if (ctx->g.nproc_t > 1) { g.slab[0] = g.V; g.slab[2] = g.V + g.XYZ; g.slab[1] = g.slab[3] = 0; /* two slices deep: never asked for (gauge_ready) */ }
  else { g.slab[0] = 0; g.slab[1] = (1 % g.T) * g.XYZ; g.slab[2] = (g.T - 1) * g.XYZ; g.slab[3] = ((g.T - 2) % g.T + g.T) % g.T * g.XYZ; }
  return g;
}

int gauge_ready(tmhip_ctx *ctx, const char *who, bool rectangles) {
  if (!ctx) TMHIP_FAIL("%s: null context", who);
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("%s: the links are not resident (tmhip_set_gauge first)", who);
  if (rectangles && ctx->g.nproc_t > 1)
    TMHIP_FAIL("%s: rectangles reach two time-slices deep and a T-split rank holds a one-deep link halo; not available with nproc_t > 1", who);
  return 0;
}

// the rank's own share of a plaquette / rectangle sum, divided by 3 as the reference does before its MPI_Allreduce; with the option
// "gauge_global_sums" the shares are added over the ranks first (one double, as square_norm with parallel = 1)
int gauge_sum(tmhip_ctx *ctx, bool rectangles, double wt, double ws, double *out) {
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const int nb = (ctx->V + 255) / 256;
  if (nb > ctx->max_partials) TMHIP_FAIL("gauge sum: partials buffer too small");
  const GaugeGeom g = gauge_geom(ctx);
  if (rectangles) hipLaunchKernelGGL(rectangle_sum_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, g, ctx->partials);
  else hipLaunchKernelGGL(plaquette_sum_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, g, wt, ws, ctx->partials);
  TMHIP_CHECK(hipGetLastError());
  double s = 0.0;
  const int global = ctx->opt_gauge_global_sums && ctx->g.nproc_t > 1;
  if (global && !ctx->comm_ready) TMHIP_FAIL("gauge sum over the ranks (\"gauge_global_sums\"): nproc_t > 1 but no communicator");
  if (tmhip_reduce_finish(ctx, nb, global, &s)) return 1;
  *out = s / 3.0;
  return 0;
}
}  // namespace gaugehip
using namespace gaugehip;

extern "C" {

int tmhip_gauge_derivative(tmhip_ctx *ctx, double beta, double c0, double c1, int use_rectangles, double glambda) {
  if (gauge_ready(ctx, "tmhip_gauge_derivative", use_rectangles != 0)) return 1;
  if (use_rectangles && c0 == 0.0) TMHIP_FAIL("tmhip_gauge_derivative: c0 = 0 with rectangles (the rectangle weight is factor c1 / c0)");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->deriv && tmhip_derivative_zero(ctx)) return 1;
  // gauge_monomial.c:50-54, :82
  const double factor = use_rectangles ? -c0 * beta / 3.0 : -1. * beta / 3.0;
  const double fr = use_rectangles ? factor * c1 / c0 : 0.0;
  const GaugeGeom g = gauge_geom(ctx);
  const dim3 grid((ctx->V + 63) / 64);
  if (use_rectangles)
    hipLaunchKernelGGL(gauge_force_kernel<true>, grid, dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, ctx->deriv, g, factor, fr, 1. + glambda, 1. - glambda);
  else
    hipLaunchKernelGGL(gauge_force_kernel<false>, grid, dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, ctx->deriv, g, factor, fr, 1. + glambda, 1. - glambda);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_measure_plaquette(tmhip_ctx *ctx, double *out) {
  if (!out) TMHIP_FAIL("tmhip_measure_plaquette: null argument");
  if (gauge_ready(ctx, "tmhip_measure_plaquette", false)) return 1;
  return gauge_sum(ctx, false, 1.0, 1.0, out);
}

int tmhip_measure_gauge_action(tmhip_ctx *ctx, double glambda, double *out) {
  if (!out) TMHIP_FAIL("tmhip_measure_gauge_action: null argument");
  if (gauge_ready(ctx, "tmhip_measure_gauge_action", false)) return 1;
  return gauge_sum(ctx, false, 1. + glambda, 1. - glambda, out);
}

int tmhip_measure_rectangles(tmhip_ctx *ctx, double *out) {
  if (!out) TMHIP_FAIL("tmhip_measure_rectangles: null argument");
  if (gauge_ready(ctx, "tmhip_measure_rectangles", true)) return 1;
  return gauge_sum(ctx, true, 1.0, 1.0, out);
}

}  // extern "C"
