// The scalars update_tm.c takes around the integrator, on the device-resident fields:
//   tmhip_moment_energy       0.5 * sum over own links of d1^2 + ... + d8^2 of the momenta        (monomial/moment_energy.c:46-74)
//   tmhip_gauge_snapshot_diff sum over own links of sqrt(|U - U_tmp|_F^2), U_tmp the snapshot       (update_tm.c:233-272)
//   tmhip_derivative_norms    sum and maximum over own links of d1^2 + ... + d8^2 of the derivative (monomial/monitor_forces.c:64-89)
// All three are one read of their fields: per-block partial sums into ctx->partials (the grid is cut to the size of that buffer and
// strides beyond it), tmhip_reduce_finish, one synchronisation.  Fixed order: two calls on the same data return the same bits.  The
// order is not the one of the reference's serial Kahan loops; every term is non-negative, so a term that passes through n additions
// and roundings on its way into the result carries a relative error of at most n 2^-53 (n per kernel: the comments below).
#include "tmhip_internal.h"

namespace {
// 256 threads -> one partial: butterfly per wave, the four waves added in order by thread 0
__device__ __forceinline__ void traj_block_store(double v, double *partials) {
  __shared__ double wsum[4];
  v = tmhip_wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
__device__ __forceinline__ double traj_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// momenta [V][4][8] doubles read as n2 = 16 V contiguous pairs, 16 bytes per lane; a block takes 1024 pairs (64 links) per sweep.
// Chain of a term: 2 (two squares and their sum) + 4 per sweep + 6 (wave) + 3 (waves of the block) + the final pass.
__global__ __launch_bounds__(256) void moment_energy_kernel(const v2d *__restrict__ p, size_t n2, double *partials) {
  double acc = 0.0;
  const size_t stride = (size_t)gridDim.x * 1024;
  for (size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x; base < n2; base += stride) {
    v2d a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { const size_t i = base + (size_t)k * 256; a[k] = i < n2 ? p[i] : v2d{0.0, 0.0}; }
#pragma unroll
    for (int k = 0; k < 4; k++) acc += a[k].x * a[k].x + a[k].y * a[k].y;
  }
  traj_block_store(acc, partials);
}

// links and snapshot ([..][4][9] complex, 144 bytes per link) read as whole contiguous rows, 16 bytes per lane: a block takes 256 links
// per sweep, every lane squares the difference of the elements it loaded into LDS and one thread per link adds the nine up (rows of
// nine doubles: conflict-free) and takes the root (_su3_minus_su3, _su3_square_norm, sqrt: update_tm.c:251-254).
// Chain of a term: 1 (difference) + 2 (squares of an element) + 9 (elements) + 1 (root) + 1 per sweep + 6 + 3 + the final pass.
__global__ __launch_bounds__(256) void snapshot_diff_kernel(const v2d *__restrict__ u, const v2d *__restrict__ w, size_t nlinks, double *partials) {
  __shared__ double sq[256 * 9];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (size_t l0 = (size_t)blockIdx.x * 256; l0 < nlinks; l0 += (size_t)gridDim.x * 256) {   // (uniform over the block)
    const int nl = (int)((nlinks - l0) < 256 ? (nlinks - l0) : 256);
#pragma unroll
    for (int j = 0; j < 9; j++) {
      const int idx = j * 256 + tid;
      if (idx < nl * 9) {
        const v2d a = u[l0 * 9 + idx], b = w[l0 * 9 + idx];
        const double dx = a.x - b.x, dy = a.y - b.y;
        sq[idx] = dx * dx + dy * dy;
      }
    }
    __syncthreads();
    if (tid < nl) {
      double s = sq[tid * 9];
#pragma unroll
      for (int e = 1; e < 9; e++) s += sq[tid * 9 + e];
      acc += sqrt(s);
    }
    __syncthreads();
  }
  traj_block_store(acc, partials);
}

// derivative [2 parities][4 mu][8][Vh]: one thread per link, the eight planes of a (parity, mu) read along the site index.  The
// per-link value is d1^2 + ... + d8^2 from left to right (_su3adj_square_norm); sums in partials[0 .. grid), maxima in pmax[0 .. grid).
// Chain of a term of the sum: 8 (link) + 1 per sweep + 6 + 3 + the final pass; the maximum is exact in the per-link values.
__global__ __launch_bounds__(256) void derivative_norms_kernel(const double *__restrict__ d, int Vh, double *partials, double *pmax) {
  __shared__ double wmax[4];
  double acc = 0.0, mx = 0.0;
  const size_t nlinks = (size_t)8 * Vh;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nlinks; j += (size_t)gridDim.x * 256) {
    const size_t pm = j / Vh, i = j - pm * Vh;
    const double *q = d + pm * 8 * Vh + i;
    double v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = q[(size_t)e * Vh];
    double s = v[0] * v[0];
#pragma unroll
    for (int e = 1; e < 8; e++) s += v[e] * v[e];
    acc += s;
    mx = fmax(mx, s);
  }
  mx = traj_wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  traj_block_store(acc, partials);   // (its barrier covers wmax)
  if (threadIdx.x == 0) pmax[blockIdx.x] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
}

__global__ __launch_bounds__(256) void max_final_kernel(const double *__restrict__ pmax, int n, double *out) {
  __shared__ double wmax[4];
  double mx = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) mx = fmax(mx, pmax[i]);
  mx = traj_wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
}

// blocks of a launch that wants `want` of them and has `rows` rows of partial sums to fill
int traj_grid(const tmhip_ctx *ctx, size_t want, int rows) {
  const size_t cap = (size_t)(ctx->max_partials / rows);
  return (int)(want < cap ? (want ? want : 1) : cap);
}
// the option "gauge_global_sums" on a T-split rank: the value over all ranks instead of the rank's share, as the gauge measures
int traj_global(tmhip_ctx *ctx, const char *who, int *global) {
  *global = ctx->opt_gauge_global_sums && ctx->g.nproc_t > 1;
  if (*global && !ctx->comm_ready) TMHIP_FAIL("%s over the ranks (\"gauge_global_sums\"): nproc_t > 1 but no communicator", who);
  return 0;
}
}  // namespace

extern "C" {

int tmhip_moment_energy(tmhip_ctx *ctx, double *out) {
  if (!out) TMHIP_FAIL("tmhip_moment_energy: null argument");
  if (!ctx->momenta) TMHIP_FAIL("tmhip_moment_energy: no momenta on the device (tmhip_momenta_upload)");
  int global = 0;
  if (traj_global(ctx, "tmhip_moment_energy", &global)) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t n2 = (size_t)ctx->V * 16;
  const int nb = traj_grid(ctx, (n2 + 1023) / 1024, 1);
  hipLaunchKernelGGL(moment_energy_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->momenta, n2, ctx->partials);
  TMHIP_CHECK(hipGetLastError());
  double s = 0.0;
  if (tmhip_reduce_finish(ctx, nb, global, &s)) return 1;
  *out = 0.5 * s;   // moment_energy.c:74
  return 0;
}

int tmhip_gauge_snapshot_diff(tmhip_ctx *ctx, double *out) {
  if (!out) TMHIP_FAIL("tmhip_gauge_snapshot_diff: null argument");
  if (!ctx->gauge_snap) TMHIP_FAIL("tmhip_gauge_snapshot_diff: no snapshot (tmhip_gauge_snapshot first)");
  if (!ctx->gauge_raw || !ctx->gauge_raw_valid) TMHIP_FAIL("tmhip_gauge_snapshot_diff: the links are not resident (tmhip_set_gauge first)");
  int global = 0;
  if (traj_global(ctx, "tmhip_gauge_snapshot_diff", &global)) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t nlinks = (size_t)ctx->V * 4;
  const int nb = traj_grid(ctx, (nlinks + 255) / 256, 1);
  hipLaunchKernelGGL(snapshot_diff_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const v2d *)ctx->gauge_raw, (const v2d *)ctx->gauge_snap, nlinks, ctx->partials);
  TMHIP_CHECK(hipGetLastError());
  return tmhip_reduce_finish(ctx, nb, global, out);
}

int tmhip_derivative_norms(tmhip_ctx *ctx, double *sum, double *max) {
  if (!sum || !max) TMHIP_FAIL("tmhip_derivative_norms: null argument");
  if (!ctx->deriv) TMHIP_FAIL("tmhip_derivative_norms: no derivative field on the device (no force has been computed)");
  int global = 0;
  if (traj_global(ctx, "tmhip_derivative_norms", &global)) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const size_t nlinks = (size_t)ctx->V * 4;
  const int nb = traj_grid(ctx, (nlinks + 255) / 256, 2);
  double *pmax = ctx->partials + ctx->max_partials / 2;   // the second row
  hipLaunchKernelGGL(derivative_norms_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const double *)ctx->deriv, ctx->Vh, ctx->partials, pmax);
  hipLaunchKernelGGL(max_final_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double *)pmax, nb, ctx->result_dev + 1);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(ctx->result_host + 1, ctx->result_dev + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (tmhip_reduce_finish(ctx, nb, global, sum)) return 1;   // synchronises
  double mx = ctx->result_host[1];
  if (global) {
    // MPI_MAX of monitor_forces.c:95 through the one sum over the ranks the transports have: rank r's value plus zeros is rank r's value
    // exactly, so np sums of one double hand every rank every rank's maximum (a monitoring call: np latencies do not matter)
    const double mine = mx;
    for (int r = 0; r < ctx->g.nproc_t; r++) {
      const double v = r == ctx->g.proc_t ? mine : 0.0;
      double got = 0.0;
      TMHIP_CHECK(hipMemcpyAsync(ctx->partials, &v, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (tmhip_reduce_finish(ctx, 1, 1, &got)) return 1;
      if (got > mx) mx = got;
    }
  }
  *max = mx;
  return 0;
}

}  // extern "C"
