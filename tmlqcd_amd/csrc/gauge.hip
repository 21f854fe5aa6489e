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
// The device functions (geometry, path product, staple sums, block reduction) are in gauge_common.h, shared with flow.hip.
#include "gauge_common.h"

namespace gaugehip {
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
// "gauge_global_sums" the shares are added over the ranks first (one double, as square_norm with parallel = 1).  links: the field
// summed over, ctx->gauge_raw or a flow buffer of flow.hip (same layout, own sites only)
int gauge_sum(tmhip_ctx *ctx, const v2d *links, bool rectangles, double wt, double ws, double *out) {
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const int nb = (ctx->V + 255) / 256;
  if (nb > ctx->max_partials) TMHIP_FAIL("gauge sum: partials buffer too small");
  const GaugeGeom g = gauge_geom(ctx);
  if (rectangles) hipLaunchKernelGGL(rectangle_sum_kernel, dim3(nb), dim3(256), 0, ctx->stream, links, g, ctx->partials);
  else hipLaunchKernelGGL(plaquette_sum_kernel, dim3(nb), dim3(256), 0, ctx->stream, links, g, wt, ws, ctx->partials);
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
  return gauge_sum(ctx, (const v2d *)ctx->gauge_raw, false, 1.0, 1.0, out);
}

int tmhip_measure_gauge_action(tmhip_ctx *ctx, double glambda, double *out) {
  if (!out) TMHIP_FAIL("tmhip_measure_gauge_action: null argument");
  if (gauge_ready(ctx, "tmhip_measure_gauge_action", false)) return 1;
  return gauge_sum(ctx, (const v2d *)ctx->gauge_raw, false, 1. + glambda, 1. - glambda, out);
}

int tmhip_measure_rectangles(tmhip_ctx *ctx, double *out) {
  if (!out) TMHIP_FAIL("tmhip_measure_rectangles: null argument");
  if (gauge_ready(ctx, "tmhip_measure_rectangles", true)) return 1;
  return gauge_sum(ctx, (const v2d *)ctx->gauge_raw, true, 1.0, 1.0, out);
}

}  // extern "C"
