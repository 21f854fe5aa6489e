// Online measurements of meas/measurements.c that are left after the gradient flow (flow.hip), fp64:
//   tmhip_slice_correlators            the per-slice bilinears of a propagator that correlators_measurement (meas/correlators.c:154-170,
//                                      time-slices) and pion_norm_measurement (meas/pion_norm.c:93-107, z-slices) add up on the host
//   tmhip_polyakov_loop                polyakov_loop_dir / polyakov_loop (meas/polyakov_loop.c:325-558, :51-157), any direction
//   tmhip_measure_oriented_plaquettes  measure_oriented_plaquettes (meas/oriented_plaquettes.c:39-86)
// The slice sums read the two e/o halves of the propagator where they lie ([12][ns] planes, site = e/o sub-index): no
// convert_eo_to_lexic, each spinor is read once (192 bytes per site) and only partial sums are written.  The two gauge measurements
// read the lexicographic resident links through the device functions of gauge_common.h.
// Reductions: every kernel leaves one partial per (value, block) in a buffer of this unit, added inside the block in a fixed order
// (butterfly within the wave and the four wave sums in order; the z-slice kernel adds the lanes of one z in lane order, see there);
// ONE final launch adds the partials of every value in the order of tmhip_block_sum256 and ONE copy brings all values of a call to the
// host: a call synchronises once however many numbers it returns, there are no floating-point atomics, and two calls give the same bits.
#include "gauge_common.h"

namespace meaship {
using namespace gaugehip;

struct MeasState {
  double *partials; size_t partials_cap;   // [values][partials per value]
  double *res_dev, *res_host; int res_cap; // one double per value; res_host is pinned
};

// value b = blockIdx.x: the sum of partials[b n .. (b + 1) n) in the fixed order of tmhip_block_sum256
__global__ __launch_bounds__(256) void meas_final_kernel(const double *__restrict__ partials, int n, double *__restrict__ out) {
  __shared__ double wsum[4];
  const double v = tmhip_block_sum256(partials + (size_t)blockIdx.x * n, n, wsum);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// NV values of a 256-thread block, value k -> partials[(first + k step) stride + slot]: the reduction of g_block_reduce_store for each
template <int NV>
__device__ __forceinline__ void block_reduce_store_n(const double (&v)[NV], double *__restrict__ partials, size_t first, size_t step, size_t stride, size_t slot) {
  __shared__ double wsum[NV][4];
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const double s = tmhip_wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) wsum[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV)
    partials[(first + threadIdx.x * step) * stride + slot] = ((wsum[threadIdx.x][0] + wsum[threadIdx.x][1]) + wsum[threadIdx.x][2]) + wsum[threadIdx.x][3];
}

// The bilinears of one site (correlators.c:165-169 with the macros of su3spinor.h): with psi = (u, l), u = spin 0, 1 and l = spin 2, 3,
//   _spinor_prod_re(psi, psi)               = |psi|^2
//   _gamma0(phi, psi): phi = (l, u)          _spinor_prod_re(psi, phi) = Re(u^+ l) + Re(l^+ u) =  2 Re B
//   _gamma5(phi, phi): phi = (l, -u)         _spinor_prod_im(psi, phi) = -Im(u^+ l) + Im(l^+ u) = -2 Im B      (_spinor_prod_im(r, s) = Im(s^+ r))
// with the one colour- and spin-pair-summed bilinear B = sum_{c < 6} conj(psi_c) psi_{c + 6}, computed once.
template <bool FULL>
__device__ __forceinline__ void site_bilinears(const v2d *__restrict__ f, int ns, int i, double &pp, double &pa, double &p4) {
  v2d c[12];
#pragma unroll
  for (int k = 0; k < 12; k++) c[k] = f[(size_t)k * ns + i];
  double n = 0.0, bre = 0.0, bim = 0.0;
#pragma unroll
  for (int k = 0; k < 12; k++) n += c[k].x * c[k].x + c[k].y * c[k].y;
  pp += n;
  if (FULL) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      bre += c[k].x * c[k + 6].x + c[k].y * c[k + 6].y;
      bim += c[k].x * c[k + 6].y - c[k].y * c[k + 6].x;
    }
    pa += 2.0 * bre;
    p4 += -2.0 * bim;
  }
}

// Time-slices.  The time-slice t of one parity is the contiguous sub-index range [t XYZ/2, (t + 1) XYZ/2) (geometry_eo.c: the e/o
// sub-index of a site is its lexicographic index / 2), so a block belongs to ONE (slice, parity) -- grid (blocks per slice, T, 2) --
// and no wave or block ever holds sites of two slices; lanes past the end of the slice add zeros.  Value q of slice t has its
// 2 gridDim.x partials at partials[(q T + t) 2 gridDim.x ...], even parity first.
template <bool FULL>
__global__ __launch_bounds__(256, 2) void slice_t_kernel(const v2d *__restrict__ even, const v2d *__restrict__ odd, int ns, int XYZh,
                                                         double *__restrict__ partials) {
  constexpr int NV = FULL ? 3 : 1;
  const int t = blockIdx.y, par = blockIdx.z, T = gridDim.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  double pp = 0.0, pa = 0.0, p4 = 0.0;
  if (j < XYZh) site_bilinears<FULL>(par ? odd : even, ns, t * XYZh + j, pp, pa, p4);
  double v[NV];
  v[0] = pp;
  if constexpr (FULL) { v[1] = pa; v[2] = p4; }
  // value q of slice t is row q T + t
  block_reduce_store_n<NV>(v, partials, (size_t)t, (size_t)T, (size_t)2 * gridDim.x, (size_t)par * gridDim.x + blockIdx.x);
}

// z-slices.  Consecutive sub-indices walk z fastest: sub-index i of parity p is the row r = i / (LZ/2) = (t, x, y) and the pair
// zh = i % (LZ/2), and its z is 2 zh + ((p + t + x + y + toff) & 1) (the site of the pair whose coordinate sum has parity p).  A block
// owns SLICE_Z_PASSES x RPP whole rows, RPP = 256 / (LZ/2): in every pass its first RPP LZ/2 threads read that many CONSECUTIVE
// sub-indices (coalesced), thread j always with the same zh = j % (LZ/2), so a thread adds up sites of two z only and keeps them
// apart in two accumulators.  Then the block adds, for every z, the RPP threads that hold it, in thread order, out of shared memory.
// Value q of slice z has its 2 gridDim.x partials at partials[(q LZ + z) 2 gridDim.x ...], even parity first.
#define SLICE_Z_PASSES 8
struct SliceZGeom { int LX, LY, LZ, rows, toff; };   // rows = T LX LY
template <bool FULL>
__global__ __launch_bounds__(256, 2) void slice_z_kernel(const v2d *__restrict__ even, const v2d *__restrict__ odd, int ns, SliceZGeom g,
                                                         double *__restrict__ partials) {
  constexpr int NV = FULL ? 3 : 1;
  __shared__ double sm[2 * NV][256];
  const int par = blockIdx.y;
  const v2d *f = par ? odd : even;
  const int H = g.LZ >> 1, rpp = 256 / H;
  const int j = threadIdx.x, zh = j % H, r0 = j / H;
  double a[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (r0 < rpp) {
    for (int pass = 0; pass < SLICE_Z_PASSES; pass++) {
      const int row = (blockIdx.x * SLICE_Z_PASSES + pass) * rpp + r0;
      if (row < g.rows) {
        const int y = row % g.LY, tx = row / g.LY, x = tx % g.LX, t = tx / g.LX;
        const int bit = (par + t + x + y + g.toff) & 1;
        double pp = 0.0, pa = 0.0, p4 = 0.0;
        site_bilinears<FULL>(f, ns, row * H + zh, pp, pa, p4);
        a[0][0] += bit ? 0.0 : pp; a[1][0] += bit ? pp : 0.0;
        if (FULL) {
          a[0][1] += bit ? 0.0 : pa; a[1][1] += bit ? pa : 0.0;
          a[0][2] += bit ? 0.0 : p4; a[1][2] += bit ? p4 : 0.0;
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int q = 0; q < NV; q++) sm[b * NV + q][j] = a[b][q];
  __syncthreads();
  const size_t stride = (size_t)2 * gridDim.x;
  for (int k = j; k < NV * g.LZ; k += 256) {
    const int q = k / g.LZ, z = k % g.LZ;
    const double *col = sm[(z & 1) * NV + q] + (z >> 1);
    double s = 0.0;
    for (int r = 0; r < rpp; r++) s += col[r * H];
    partials[(size_t)k * stride + (size_t)par * gridDim.x + blockIdx.x] = s;
  }
}

// One thread per line along `dir`: the ordered product of its L links from coordinate 0, left to right with gaugehip::mm as
// polyakov_loop.c:366-392 multiplies, and the trace.  Lines are numbered lexicographically over the other three coordinates.
// partials[b] = block b's sum of Re tr, partials[nb + b] of Im tr.
__global__ __launch_bounds__(256, 2) void polyakov_kernel(const v2d *__restrict__ raw, GaugeGeom g, int dir, int L, int lines,
                                                          double *__restrict__ partials, int nb) {
  const int line = blockIdx.x * 256 + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (line < lines) {
    const int ext[4] = {g.T, g.LX, g.LY, g.LZ};
    int co[4], r = line;
#pragma unroll
    for (int d = 3; d >= 0; d--) {
      if (d == dir) { co[d] = 0; continue; }
      co[d] = r % ext[d];
      r /= ext[d];
    }
    Site s{co[0], co[1], co[2], co[3]};
    cd acc[9];
    g_load(acc, raw, g, s, dir);
#pragma unroll 1
    for (int k = 1; k < L; k++) {
      s = g_shift(s, dir, 1);
      cd l[9], t[9];
      g_load(l, raw, g, s, dir);
      mm(t, acc, l);
#pragma unroll
      for (int e = 0; e < 9; e++) acc[e] = t[e];
    }
    v[0] = (acc[0].x + acc[4].x) + acc[8].x;
    v[1] = (acc[0].y + acc[4].y) + acc[8].y;
  }
  block_reduce_store_n<2>(v, partials, 0, 1, (size_t)nb, blockIdx.x);
}

// The per-site work of plaquette_sum_kernel (gauge.hip) with one accumulator per plane instead of one weighted sum: plane p of
// (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) is Re tr( U_mu1(x) U_mu2(x+mu1) [U_mu2(x) U_mu1(x+mu2)]^dagger ), oriented_plaquettes.c:52-72.
// The loop over the planes stays rolled (as there: unrolled, the 24 link loads are gathered in front of the products); a plane's
// value is moved into its own scalar by a select.  partials[p nb + b] = block b's sum of plane p.
__global__ __launch_bounds__(256, 2) void oriented_plaquette_kernel(const v2d *__restrict__ raw, GaugeGeom g, double *__restrict__ partials, int nb) {
  const int ix = blockIdx.x * 256 + threadIdx.x;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (ix < g.V) {
    const Site s = g_site(g, ix);
    int plane = 0;
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
        const double pl = retr_mmd(p1, p2);
#pragma unroll
        for (int p = 0; p < 6; p++) v[p] = plane == p ? pl : v[p];
        plane++;
      }
  }
  block_reduce_store_n<6>(v, partials, 0, 1, (size_t)nb, blockIdx.x);
}

static MeasState *meas_state(tmhip_ctx *ctx) {
  if (!ctx->meas) {
    MeasState *st = new (std::nothrow) MeasState();
    if (!st) return nullptr;
    st->partials = nullptr; st->partials_cap = 0; st->res_dev = st->res_host = nullptr; st->res_cap = 0;
    ctx->meas = st;
  }
  return (MeasState *)ctx->meas;
}
// room for `nval` values of `per` partials each; buffers only ever grow
static int meas_reserve(tmhip_ctx *ctx, int nval, size_t per, MeasState **out) {
  MeasState *st = meas_state(ctx);
  if (!st) TMHIP_FAIL("online measurements: out of host memory");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t need = (size_t)nval * per;
  if (need > st->partials_cap) {
    if (st->partials) { TMHIP_CHECK(hipStreamSynchronize(ctx->stream)); (void)hipFree(st->partials); st->partials = nullptr; st->partials_cap = 0; }
    TMHIP_CHECK(hipMalloc((void **)&st->partials, need * sizeof(double)));
    st->partials_cap = need;
  }
  if (nval > st->res_cap) {
    if (st->res_dev) { TMHIP_CHECK(hipStreamSynchronize(ctx->stream)); (void)hipFree(st->res_dev); (void)hipHostFree(st->res_host); st->res_dev = st->res_host = nullptr; st->res_cap = 0; }
    TMHIP_CHECK(hipMalloc((void **)&st->res_dev, (size_t)nval * sizeof(double)));
    if (hipHostMalloc((void **)&st->res_host, (size_t)nval * sizeof(double)) != hipSuccess) {
      (void)hipFree(st->res_dev);
      st->res_dev = st->res_host = nullptr;
      TMHIP_FAIL("online measurements: no pinned memory for %d results", nval);
    }
    st->res_cap = nval;
  }
  *out = st;
  return 0;
}
// the final pass over `per` partials of each of `nval` values, the copy of all of them and the call's one synchronisation
static int meas_finish(tmhip_ctx *ctx, MeasState *st, int nval, size_t per) {
  hipLaunchKernelGGL(meas_final_kernel, dim3(nval), dim3(256), 0, ctx->stream, (const double *)st->partials, (int)per, st->res_dev);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(st->res_host, st->res_dev, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}
static int meas_unsplit(tmhip_ctx *ctx, const char *who) {
  if (gauge_ready(ctx, who, false)) return 1;
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("%s: a line or a plaquette of a T-split rank crosses to its neighbours; not available with nproc_t > 1", who);
  return 0;
}
}  // namespace meaship
using namespace meaship;

void tmhip_meas_destroy(tmhip_ctx *ctx) {
  MeasState *st = (MeasState *)ctx->meas;
  if (!st) return;
  if (st->partials) (void)hipFree(st->partials);
  if (st->res_dev) (void)hipFree(st->res_dev);
  if (st->res_host) (void)hipHostFree(st->res_host);
  delete st;
  ctx->meas = nullptr;
}

extern "C" {

int tmhip_slice_correlators(tmhip_ctx *ctx, const tmhip_field *even, const tmhip_field *odd, int dir, double *pp, double *pa, double *p4) {
  if (!ctx || !even || !odd || !pp) TMHIP_FAIL("tmhip_slice_correlators: null argument");
  if (dir != 0 && dir != 3) TMHIP_FAIL("tmhip_slice_correlators: dir = %d, must be 0 (time-slices) or 3 (z-slices)", dir);
  if (even->kind != TMHIP_FIELD_EO || odd->kind != TMHIP_FIELD_EO) TMHIP_FAIL("tmhip_slice_correlators: needs the two one-parity (EO) halves, not a FULL field");
  if (even->prec != 0 || odd->prec != 0) TMHIP_FAIL("tmhip_slice_correlators: fp64 fields only (an fp32 propagator is not summed)");
  if (even->ns != ctx->ns || odd->ns != ctx->ns) TMHIP_FAIL("tmhip_slice_correlators: field of another context");
  const bool full = pa || p4;   // the two are the parts of one bilinear: computed together, each copied out if asked for
  const int nq = full ? 3 : 1;
  const int nslice = dir == 0 ? ctx->g.T : ctx->g.LZ;
  MeasState *st = nullptr;
  size_t per;
  if (dir == 0) {
    const int XYZh = ctx->face;
    const int nbx = (XYZh + 255) / 256;
    per = (size_t)2 * nbx;
    if (meas_reserve(ctx, nq * nslice, per, &st)) return 1;
    const dim3 grid(nbx, ctx->g.T, 2);
    if (full) hipLaunchKernelGGL(slice_t_kernel<true>, grid, dim3(256), 0, ctx->stream, (const v2d *)even->d, (const v2d *)odd->d, ctx->ns, XYZh, st->partials);
    else hipLaunchKernelGGL(slice_t_kernel<false>, grid, dim3(256), 0, ctx->stream, (const v2d *)even->d, (const v2d *)odd->d, ctx->ns, XYZh, st->partials);
  } else {
    const int H = ctx->g.LZ / 2;
    if (H > 256) TMHIP_FAIL("tmhip_slice_correlators: LZ = %d, z-slices are summed for LZ <= 512", ctx->g.LZ);
    SliceZGeom g;
    g.LX = ctx->g.LX; g.LY = ctx->g.LY; g.LZ = ctx->g.LZ; g.rows = ctx->g.T * ctx->g.LX * ctx->g.LY; g.toff = ctx->g.proc_t * ctx->g.T;
    const int rows_per_block = SLICE_Z_PASSES * (256 / H);
    const int nbx = (g.rows + rows_per_block - 1) / rows_per_block;
    per = (size_t)2 * nbx;
    if (meas_reserve(ctx, nq * nslice, per, &st)) return 1;
    const dim3 grid(nbx, 2);
    if (full) hipLaunchKernelGGL(slice_z_kernel<true>, grid, dim3(256), 0, ctx->stream, (const v2d *)even->d, (const v2d *)odd->d, ctx->ns, g, st->partials);
    else hipLaunchKernelGGL(slice_z_kernel<false>, grid, dim3(256), 0, ctx->stream, (const v2d *)even->d, (const v2d *)odd->d, ctx->ns, g, st->partials);
  }
  if (meas_finish(ctx, st, nq * nslice, per)) return 1;
  memcpy(pp, st->res_host, nslice * sizeof(double));
  if (pa) memcpy(pa, st->res_host + nslice, nslice * sizeof(double));
  if (p4) memcpy(p4, st->res_host + 2 * nslice, nslice * sizeof(double));
  return 0;   // site-local: no exchange was waited for, so there is nothing of the halo machinery to check (and no second synchronisation)
}

int tmhip_polyakov_loop(tmhip_ctx *ctx, int dir, double *re, double *im) {
  if (!re || !im) TMHIP_FAIL("tmhip_polyakov_loop: null argument");
  if (meas_unsplit(ctx, "tmhip_polyakov_loop")) return 1;
  if (dir < 0 || dir > 3) TMHIP_FAIL("tmhip_polyakov_loop: dir = %d, must be 0 .. 3", dir);
  const int ext[4] = {ctx->g.T, ctx->g.LX, ctx->g.LY, ctx->g.LZ};
  const int L = ext[dir];
  if (L < 3) TMHIP_FAIL("tmhip_polyakov_loop: extent %d along dir %d (the reference's loop multiplies three links there; not reproduced)", L, dir);
  const int lines = ctx->V / L;
  const int nb = (lines + 255) / 256;
  MeasState *st = nullptr;
  if (meas_reserve(ctx, 2, (size_t)nb, &st)) return 1;
  hipLaunchKernelGGL(polyakov_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, gauge_geom(ctx), dir, L, lines, st->partials, nb);
  if (meas_finish(ctx, st, 2, (size_t)nb)) return 1;
  /* polyakov_loop.c:537: pl /= 3 VOLUME3 */
  *re = st->res_host[0] / (3. * lines);
  *im = st->res_host[1] / (3. * lines);
  return 0;
}

int tmhip_measure_oriented_plaquettes(tmhip_ctx *ctx, double plaq[6]) {
  if (!plaq) TMHIP_FAIL("tmhip_measure_oriented_plaquettes: null argument");
  if (meas_unsplit(ctx, "tmhip_measure_oriented_plaquettes")) return 1;
  const int nb = (ctx->V + 255) / 256;
  MeasState *st = nullptr;
  if (meas_reserve(ctx, 6, (size_t)nb, &st)) return 1;
  hipLaunchKernelGGL(oriented_plaquette_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, gauge_geom(ctx), st->partials, nb);
  if (meas_finish(ctx, st, 6, (size_t)nb)) return 1;
  /* oriented_plaquettes.c:75-78 with g_nproc = 1 */
  for (int j = 0; j < 6; j++) plaq[j] = (st->res_host[j] / 3.0) / ctx->V;
  return 0;
}

}  // extern "C"
