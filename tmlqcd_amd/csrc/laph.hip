// LapH eigensystem on the device (gfx950): the gauge-covariant 3D Laplacian of jacobi.c on colour vectors, and a thick-restart Lanczos
// whose every kernel carries the time-slice as a grid dimension -- T independent eigenproblems of LX LY LZ sites advance in lock-step.
// It stands where the reference has LapH_ev.c over solver/eigenvalues_Jacobi.c (Jacobi-Davidson on LAPACK, one slice after the other
// on host vectors).  Per slice the algorithm is that of eig.hip (tests/eig_restate.py).
//
// A colour-vector field: v2d d[3][cs], plane = colour, site = t S3 + ix (lexicographic, the host's order), cs = VOLUME rounded up to 64;
// a time-slice is the contiguous range [t S3, (t + 1) S3) of every plane.  The links are read from the lexicographic resident copy
// (ctx->gauge_raw, [site][mu][9]) like the gauge measurements do.
//
//   laph_kernel<MODE>    one thread per site of a slice, grid (blocks of a slice, slices): 0 out = A in; 1 the same and block sums of
//                        <in, out>; 2 out = c1 (A in) + c2 in + c3 prev with the coefficients of the slice read from the device
//   laph_dots_kernel     h_i = <v_i, w>, i < nv <= 65, per slice: w once, every v_i once (eig_dots_kernel with a slice dimension)
//   laph_project_kernel  w -= sum_i h_i v_i ascending i, block sums of |w|^2 in the pass
//   laph_scale_kernel    out = w / sqrt(|w|^2), the norm of the slice read from the device
//   laph_rotate_kernel   V[:, 0:k] = V[:, 0:n] Y_t in place: a thread owns ONE real number of a plane across all n vectors, parks its
//                        n values in LDS and forms the k columns in groups of 16 accumulators
//   laph_comb_kernel     out = c1 x + c2 y + c3 z, per-slice coefficients: the filter's own pass with "laph_fused" 0
// Every kernel takes the set of active slices BY VALUE (a 256-bit mask): a block of a frozen slice returns at once.
// Sums: one partial per block (butterfly in the wave, the wave sums in order), then laph_final_kernel adds the partials of every
// (slice, value) in a fixed tree: the same bits from call to call, no floating-point atomics.
#include "gauge_common.h"
#include "eig_small.h"
#include <vector>
#include <algorithm>
#include <thread>
#include <chrono>

struct tmhip_cvfield {
  v2d *d;          // [3][cs]
  int cs;          // plane stride
  tmhip_ctx *ctx;  // the context it belongs to
};

namespace laphhip {

#define LAPH_NV 65                           // vectors per launch of the dots / the projection
#define LAPH_NB (TMHIP_LAPH_MAX_BASIS + 1)   // vectors of a basis: m and the residual vector
#define LAPH_MAX_SLICES 256
#define LAPH_HOST_THREADS 16                 // host threads over the small eigenproblems of a restart: a constant, never the machine's CPU count

struct Mask {
  unsigned long long w[LAPH_MAX_SLICES / 64];
  __host__ __device__ bool on(int i) const { return (w[i >> 6] >> (i & 63)) & 1ull; }
};
struct Geom { int LX, LY, LZ, S3, cs; };
struct Vecs { const v2d *v[LAPH_NV]; };
struct Basis { v2d *v[TMHIP_LAPH_MAX_BASIS]; };

// ---- the operator ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_link(v2d (&u)[9], const v2d *__restrict__ raw, size_t site, int mu) {
  const v2d *p = raw + (site * 4 + mu) * 9;
#pragma unroll
  for (int e = 0; e < 9; e++) u[e] = p[e];
}
// a * b and conj(a) * b
__device__ __forceinline__ v2d cmul(v2d a, v2d b) { return v2d{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ v2d cmulc(v2d a, v2d b) { return v2d{a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x}; }

template <int MODE>
__global__ __launch_bounds__(256, 3) void laph_kernel(const v2d *__restrict__ raw, const v2d *__restrict__ in, v2d *__restrict__ out,
                                                      const v2d *__restrict__ prev, const double *__restrict__ coef, Geom g, int t0, Mask active,
                                                      double *__restrict__ partials) {
  const int ts = blockIdx.y;
  if (!active.on(ts)) return;
  const int ix = blockIdx.x * 256 + threadIdx.x;
  double dre = 0.0, dim = 0.0;
  if (ix < g.S3) {
    const int z = ix % g.LZ, r = ix / g.LZ, y = r % g.LY, x = r / g.LY;
    const size_t base = (size_t)(t0 + ts) * g.S3;
    // g_iup3d / g_idn3d of geometry_eo.c:851-860: the neighbours inside the slice
    const int up[3] = {ix + (x + 1 < g.LX ? 1 : 1 - g.LX) * g.LY * g.LZ, ix + (y + 1 < g.LY ? 1 : 1 - g.LY) * g.LZ, ix + (z + 1 < g.LZ ? 1 : 1 - g.LZ)};
    const int dn[3] = {ix - (x > 0 ? 1 : 1 - g.LX) * g.LY * g.LZ, ix - (y > 0 ? 1 : 1 - g.LY) * g.LZ, ix - (z > 0 ? 1 : 1 - g.LZ)};
    const v2d *k = in + base;
    v2d k0[3], l[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { k0[c] = k[(size_t)c * g.cs + ix]; l[c] = v2d{6.0 * k0[c].x, 6.0 * k0[c].y}; }
#pragma unroll
    for (int mu = 0; mu < 3; mu++) {
      v2d u[9], s[3];
      // _su3_multiply(lt, U_mu(x), k(x + mu)); l -= lt
      load_link(u, raw, base + ix, mu + 1);
#pragma unroll
      for (int c = 0; c < 3; c++) s[c] = k[(size_t)c * g.cs + up[mu]];
#pragma unroll
      for (int c = 0; c < 3; c++) l[c] -= cmul(u[3 * c], s[0]) + cmul(u[3 * c + 1], s[1]) + cmul(u[3 * c + 2], s[2]);
      // _su3_inverse_multiply(lt, U_mu(x - mu), k(x - mu)); l -= lt
      load_link(u, raw, base + dn[mu], mu + 1);
#pragma unroll
      for (int c = 0; c < 3; c++) s[c] = k[(size_t)c * g.cs + dn[mu]];
#pragma unroll
      for (int c = 0; c < 3; c++) l[c] -= cmulc(u[c], s[0]) + cmulc(u[3 + c], s[1]) + cmulc(u[6 + c], s[2]);
    }
    if (MODE == 2) {
      const double c1 = coef[3 * ts], c2 = coef[3 * ts + 1];
#pragma unroll
      for (int c = 0; c < 3; c++) l[c] = v2d{c1 * l[c].x + c2 * k0[c].x, c1 * l[c].y + c2 * k0[c].y};
      if (prev) {
        const double c3 = coef[3 * ts + 2];
#pragma unroll
        for (int c = 0; c < 3; c++) { const v2d p = prev[base + (size_t)c * g.cs + ix]; l[c] = v2d{l[c].x + c3 * p.x, l[c].y + c3 * p.y}; }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out[base + (size_t)c * g.cs + ix] = l[c];
    if (MODE == 1) {
#pragma unroll
      for (int c = 0; c < 3; c++) tmhip_cdot_add(dre, dim, k0[c], l[c]);
    }
  }
  if (MODE == 1) {
    __shared__ double wsum[2][4];
    const double a = tmhip_wave_sum(dre), b = tmhip_wave_sum(dim);
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = a; wsum[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x < 2)
      partials[((size_t)ts * 2 + threadIdx.x) * gridDim.x + blockIdx.x] = ((wsum[threadIdx.x][0] + wsum[threadIdx.x][1]) + wsum[threadIdx.x][2]) + wsum[threadIdx.x][3];
  }
}

// ---- the vector kernels: grid (blocks of a plane of a slice, 3 planes, slices) ---------------------------------------------------
// value k = blockIdx.x of nvals of slice blockIdx.y: the `per` block sums added in a fixed tree -> out[slice ostride + k]
__global__ __launch_bounds__(256) void laph_final_kernel(const double *__restrict__ partials, int per, int nvals, double *__restrict__ out, int ostride, Mask active) {
  __shared__ double sm[256];
  const int ts = blockIdx.y;
  if (!active.on(ts)) return;
  const double *p = partials + ((size_t)ts * nvals + blockIdx.x) * per;
  double acc = 0.0;
  for (int i = threadIdx.x; i < per; i += 256) acc += p[i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int q = 128; q > 0; q >>= 1) {
    if ((int)threadIdx.x < q) sm[threadIdx.x] += sm[threadIdx.x + q];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(size_t)ts * ostride + blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(LA_BS, 8) void laph_dots_kernel(const Vecs V, int nv, const v2d *__restrict__ W, Geom g, int t0, Mask active, double *__restrict__ partials) {
  __shared__ double wsum[2 * LAPH_NV][LA_BS / 64];
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const size_t off = (size_t)blockIdx.y * g.cs + (size_t)(t0 + ts) * g.S3;
  const v2d *w = W + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x, n = g.S3;
  v2d b[LA_UNROLL];
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) b[u] = base + u * LA_BS < n ? w[base + u * LA_BS] : v2d{0.0, 0.0};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = 0; i < nv; i++) {
    const v2d *vi = V.v[i] + off;
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int u = 0; u < LA_UNROLL; u++)
      if (base + u * LA_BS < n) tmhip_cdot_add(re, im, vi[base + u * LA_BS], b[u]);
    const double a = tmhip_wave_sum(re), c = tmhip_wave_sum(im);
    if (lane == 0) { wsum[2 * i][wv] = a; wsum[2 * i + 1][wv] = c; }
  }
  __syncthreads();
  const size_t per = (size_t)gridDim.x * gridDim.y;
  for (int k = threadIdx.x; k < 2 * nv; k += LA_BS) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < LA_BS / 64; q++) t += wsum[k][q];
    partials[((size_t)ts * 2 * nv + k) * per + blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// h of slice ts at h[ts hstride ..], nv complex coefficients
__global__ __launch_bounds__(LA_BS, 8) void laph_project_kernel(const Vecs V, int nv, v2d *__restrict__ W, const double *__restrict__ h, int hstride, Geom g,
                                                                int t0, Mask active, double *__restrict__ partials) {
  __shared__ double wsum[LA_BS / 64];
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const size_t off = (size_t)blockIdx.y * g.cs + (size_t)(t0 + ts) * g.S3;
  v2d *w = W + off;
  const double *hs = h + (size_t)ts * hstride;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x, n = g.S3;
  v2d b[LA_UNROLL];
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) b[u] = base + u * LA_BS < n ? w[base + u * LA_BS] : v2d{0.0, 0.0};
#pragma unroll 2
  for (int i = 0; i < nv; i++) {
    const v2d *vi = V.v[i] + off;
    const double cre = hs[2 * i], cim = hs[2 * i + 1];
#pragma unroll
    for (int u = 0; u < LA_UNROLL; u++)
      if (base + u * LA_BS < n) b[u] = tmhip_sub_cmul(b[u], cre, cim, vi[base + u * LA_BS]);
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++)
    if (base + u * LA_BS < n) { if (nv) w[base + u * LA_BS] = b[u]; acc += b[u].x * b[u].x + b[u].y * b[u].y; }
  acc = tmhip_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < LA_BS / 64; q++) t += wsum[q];
    partials[(size_t)ts * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// out = in / sqrt(nrm2 of the slice) (zero for a slice of norm zero: the breakdown is the host's to see); out may be in
__global__ __launch_bounds__(LA_BS, 8) void laph_scale_kernel(v2d *__restrict__ O, const v2d *__restrict__ I, const double *__restrict__ nrm2, int nstride, Geom g, int t0,
                                                              Mask active) {
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const size_t off = (size_t)blockIdx.y * g.cs + (size_t)(t0 + ts) * g.S3;
  const double q = nrm2[(size_t)ts * nstride], c = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < g.S3) { const v2d a = I[off + i]; O[off + i] = v2d{c * a.x, c * a.y}; }
  }
}

// out = c1 x + c2 y [+ c3 z], coef[3 ts ..] = (c1, c2, c3); x == nullptr: out = y (the masked copy).  Element-wise: out may be any input
__global__ __launch_bounds__(LA_BS, 8) void laph_comb_kernel(v2d *__restrict__ O, const v2d *X, const v2d *Y, const v2d *Z, const double *__restrict__ coef, Geom g, int t0,
                                                             Mask active) {
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const size_t off = (size_t)blockIdx.y * g.cs + (size_t)(t0 + ts) * g.S3;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
  if (!X) {
#pragma unroll
    for (int u = 0; u < LA_UNROLL; u++) {
      const int i = base + u * LA_BS;
      if (i < g.S3) O[off + i] = Y[off + i];
    }
    return;
  }
  const double c1 = coef[3 * ts], c2 = coef[3 * ts + 1], c3 = Z ? coef[3 * ts + 2] : 0.0;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < g.S3) {
      const v2d a = X[off + i], b = Y[off + i];
      v2d r = v2d{c1 * a.x + c2 * b.x, c1 * a.y + c2 * b.y};
      if (Z) { const v2d c = Z[off + i]; r = v2d{r.x + c3 * c.x, r.y + c3 * c.y}; }
      O[off + i] = r;
    }
  }
}

// V[:, 0:k] = V[:, 0:n] Y_t, Y real: Y of slice ts lies at Y[ts n KP ..] as n rows of KP doubles, KP = k rounded up to 16, zero beyond
// column k.  A thread owns one REAL number (Y is real: real and imaginary parts rotate alike) of a plane of a slice across all n
// vectors: it parks the n values in its own column of LDS (n x 64 doubles per one-wave block, read back without bank conflicts),
// forms 16 columns at a time in registers -- the row of Y is uniform and arrives through scalar loads -- and stores each group after
// the last read of its inputs from LDS: in place, no work field, any k <= n <= 128.
#define LAPH_RG 16
__global__ __launch_bounds__(64) void laph_rotate_kernel(const Basis V, int n, int k, const double *__restrict__ Y, int KP, Geom g, int t0, Mask active) {
  extern __shared__ double sm[];
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const int lane = threadIdx.x, e = blockIdx.x * 64 + lane;
  const bool valid = e < 2 * g.S3;
  const size_t off = 2 * ((size_t)blockIdx.y * g.cs + (size_t)(t0 + ts) * g.S3) + e;
  for (int i = 0; i < n; i++) sm[i * 64 + lane] = valid ? ((const double *)V.v[i])[off] : 0.0;
  const double *Yt = Y + (size_t)ts * n * KP;
  for (int c0 = 0; c0 < k; c0 += LAPH_RG) {
    double acc[LAPH_RG];
#pragma unroll
    for (int c = 0; c < LAPH_RG; c++) acc[c] = 0.0;
#pragma unroll 2
    for (int i = 0; i < n; i++) {
      const double a = sm[i * 64 + lane];
      const double *y = Yt + (size_t)i * KP + c0;
#pragma unroll
      for (int c = 0; c < LAPH_RG; c++) acc[c] = __builtin_fma(y[c], a, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < LAPH_RG; c++)
      if (c0 + c < k && valid) ((double *)V.v[c0 + c])[off] = acc[c];
  }
}

// the default start vector: a fixed pseudo-random fill in (-1, 1), a hash of (plane, site of the lattice) -- the same on every call
__global__ __launch_bounds__(LA_BS) void laph_fill_kernel(v2d *__restrict__ O, Geom g, int t0, Mask active) {
  const int ts = blockIdx.z;
  if (!active.on(ts)) return;
  const int e = blockIdx.x * LA_BS + threadIdx.x;
  if (e >= g.S3) return;
  const size_t site = (size_t)(t0 + ts) * g.S3 + e;
  unsigned long long z = ((unsigned long long)blockIdx.y << 40) + site + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const double re = (double)(unsigned)(z & 0xffffffffu) * (2.0 / 4294967296.0) - 1.0 + 1.0 / 4294967296.0;
  const double im = (double)(unsigned)(z >> 32) * (2.0 / 4294967296.0) - 1.0 + 1.0 / 4294967296.0;
  O[(size_t)blockIdx.y * g.cs + site] = v2d{re, im};
}

// host [n][3] <-> n consecutive sites of the planes
template <bool UP>
__global__ __launch_bounds__(256) void cv_layout_kernel(v2d *__restrict__ aos, v2d *__restrict__ soa, int cs, int V) {
  const int tid = blockIdx.x * 256 + threadIdx.x;
  if (tid >= 3 * V) return;
  const int site = tid / 3, c = tid % 3;
  if (UP) soa[(size_t)c * cs + site] = aos[tid];
  else aos[tid] = soa[(size_t)c * cs + site];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Work {
  std::vector<tmhip_cvfield *> v;   // basis (m + 1) and two work vectors
  double *partials, *res_dev, *res_host, *y_dev, *coef_dev;
  size_t res_len, y_len;
  double lo, hi;                    // tmhip_laph_set_interval (0, 0: automatic)
  double small_s, total_s;          // host seconds of the last tmhip_laph_eigensystem in the small eigenproblems / in all (tmhip_laph_timing)
};

static Geom geom_of(const tmhip_ctx *ctx) {
  Geom g;
  g.LX = ctx->g.LX; g.LY = ctx->g.LY; g.LZ = ctx->g.LZ; g.S3 = g.LX * g.LY * g.LZ; g.cs = (ctx->V + 63) / 64 * 64;
  return g;
}
static int stream_blocks(const Geom &g) { return (g.S3 + LA_BS * LA_UNROLL - 1) / (LA_BS * LA_UNROLL); }
static dim3 stream_grid(const Geom &g, int nt) { return dim3(stream_blocks(g), 3, nt); }

static Work *work_of(tmhip_ctx *ctx) {
  if (!ctx->laph) {
    Work *w = new Work();
    w->partials = w->res_dev = w->res_host = w->y_dev = w->coef_dev = nullptr;
    w->res_len = w->y_len = 0; w->lo = w->hi = 0.0; w->small_s = w->total_s = 0.0;
    ctx->laph = w;
  }
  return (Work *)ctx->laph;
}

static void destroy(tmhip_ctx *ctx) {
  Work *w = (Work *)ctx->laph;
  if (!w) return;
  for (tmhip_cvfield *f : w->v) tmhip_cvfield_free(ctx, f);
  if (w->partials) (void)hipFree(w->partials);
  if (w->res_dev) (void)hipFree(w->res_dev);
  if (w->y_dev) (void)hipFree(w->y_dev);
  if (w->coef_dev) (void)hipFree(w->coef_dev);
  if (w->res_host) (void)hipHostFree(w->res_host);
  delete w;
  ctx->laph = nullptr;
}

// partial sums of the widest launch (a chunk of dots over all T slices), the coefficients of the filter, `res` doubles of results on
// the device and pinned on the host, `ylen` doubles of rotation matrices; buffers only ever grow
static int buffers(tmhip_ctx *ctx, Work *w, size_t res, size_t ylen) {
  const Geom g = geom_of(ctx);
  if (!w->partials) {
    const size_t per = std::max((size_t)3 * stream_blocks(g), (size_t)(g.S3 + 255) / 256);
    TMHIP_CHECK(hipMalloc((void **)&w->partials, (size_t)ctx->g.T * 2 * LAPH_NV * per * sizeof(double)));
    TMHIP_CHECK(hipMalloc((void **)&w->coef_dev, (size_t)2 * ctx->g.T * 3 * sizeof(double)));
    TMHIP_CHECK(hipFuncSetAttribute((const void *)laph_rotate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TMHIP_LAPH_MAX_BASIS * 64 * (int)sizeof(double)));
  }
  if (res > w->res_len) {
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (w->res_dev) { (void)hipFree(w->res_dev); (void)hipHostFree(w->res_host); w->res_dev = w->res_host = nullptr; w->res_len = 0; }
    TMHIP_CHECK(hipMalloc((void **)&w->res_dev, res * sizeof(double)));
    TMHIP_CHECK(hipHostMalloc((void **)&w->res_host, res * sizeof(double)));
    w->res_len = res;
  }
  if (ylen > w->y_len) {
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (w->y_dev) { (void)hipFree(w->y_dev); w->y_dev = nullptr; w->y_len = 0; }
    TMHIP_CHECK(hipMalloc((void **)&w->y_dev, ylen * sizeof(double)));
    w->y_len = ylen;
  }
  return 0;
}

static int reserve(tmhip_ctx *ctx, Work *w, int count) {
  while ((int)w->v.size() < count) {
    tmhip_cvfield *f = nullptr;
    if (tmhip_cvfield_alloc(ctx, &f)) return 1;
    w->v.push_back(f);
  }
  return 0;
}

static Mask mask_all(int nt) {
  Mask m;
  memset(&m, 0, sizeof(m));
  for (int i = 0; i < nt; i++) m.w[i >> 6] |= 1ull << (i & 63);
  return m;
}
static Mask mask_from(const int *active, int nt) {
  if (!active) return mask_all(nt);
  Mask m;
  memset(&m, 0, sizeof(m));
  for (int i = 0; i < nt; i++) if (active[i]) m.w[i >> 6] |= 1ull << (i & 63);
  return m;
}
static bool mask_any(const Mask &m) { return (m.w[0] | m.w[1] | m.w[2] | m.w[3]) != 0; }

// ---- refusals
static int unsplit(tmhip_ctx *ctx, const char *who) {
  if (!ctx) TMHIP_FAIL("%s: null context", who);
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: T-split ranks (and their loopback rehearsal) are not built: a colour-vector field holds whole time-slices of one rank", who);
  return 0;
}
static int with_links(tmhip_ctx *ctx, const char *who) {
  if (unsplit(ctx, who)) return 1;
  return gaugehip::gauge_ready(ctx, who, false);
}
static int slices_ok(tmhip_ctx *ctx, const char *who, int t0, int nt) {
  if (t0 < 0 || nt < 1 || t0 > ctx->g.T - nt) TMHIP_FAIL("%s: time-slices [%d, %d) are outside [0, T = %d)", who, t0, t0 + nt, ctx->g.T);
  return 0;
}
static int range_ok(tmhip_ctx *ctx, const char *who, int t0, int nt) {
  if (slices_ok(ctx, who, t0, nt)) return 1;
  if (nt > LAPH_MAX_SLICES) TMHIP_FAIL("%s: %d time-slices, a call takes at most %d", who, nt, LAPH_MAX_SLICES);
  return 0;
}
static int field_ok(tmhip_ctx *ctx, const char *who, const tmhip_cvfield *f, const char *name) {
  if (!f) TMHIP_FAIL("%s: %s is null", who, name);
  if (f->ctx != ctx) TMHIP_FAIL("%s: %s is a field of another context", who, name);
  return 0;
}

// ---- the pieces, enqueued on ctx->stream: results stay on the device
struct Launch { tmhip_ctx *ctx; Work *w; Geom g; int t0, nt; };

// MODE 0 / 1 / 2 of laph_kernel with "laph_fused" 1; with 0 the plain operator and a pass of its own.  dots_dev: (re, im) of slice
// ts at dots_dev[ts dstride ..]; coef_dev: [nt][3]
static int enqueue_apply(const Launch &L, int fused, int mode, v2d *out, const v2d *in, const v2d *prev, const double *coef_dev, double *dots_dev, int dstride,
                         const Mask &mask) {
  tmhip_ctx *ctx = L.ctx;
  const dim3 grid((L.g.S3 + 255) / 256, L.nt);
  const v2d *raw = ctx->gauge_raw;
  if (mode == 0 || !fused) hipLaunchKernelGGL(laph_kernel<0>, grid, dim3(256), 0, ctx->stream, raw, in, out, (const v2d *)nullptr, (const double *)nullptr, L.g, L.t0, mask, (double *)nullptr);
  if (mode == 1) {
    if (fused) {
      hipLaunchKernelGGL(laph_kernel<1>, grid, dim3(256), 0, ctx->stream, raw, in, out, (const v2d *)nullptr, (const double *)nullptr, L.g, L.t0, mask, L.w->partials);
      hipLaunchKernelGGL(laph_final_kernel, dim3(2, L.nt), dim3(256), 0, ctx->stream, (const double *)L.w->partials, (int)grid.x, 2, dots_dev, dstride, mask);
    } else {
      Vecs V;
      memset(&V, 0, sizeof(V));
      V.v[0] = in;
      const dim3 sg = stream_grid(L.g, L.nt);
      hipLaunchKernelGGL(laph_dots_kernel, sg, dim3(LA_BS), 0, ctx->stream, V, 1, (const v2d *)out, L.g, L.t0, mask, L.w->partials);
      hipLaunchKernelGGL(laph_final_kernel, dim3(2, L.nt), dim3(256), 0, ctx->stream, (const double *)L.w->partials, (int)(sg.x * sg.y), 2, dots_dev, dstride, mask);
    }
  }
  if (mode == 2) {
    if (fused) hipLaunchKernelGGL(laph_kernel<2>, grid, dim3(256), 0, ctx->stream, raw, in, out, prev, coef_dev, L.g, L.t0, mask, (double *)nullptr);
    else hipLaunchKernelGGL(laph_comb_kernel, stream_grid(L.g, L.nt), dim3(LA_BS), 0, ctx->stream, out, (const v2d *)out, in, prev, coef_dev, L.g, L.t0, mask);
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// <v_i, w>, i < nv, of slice ts -> out_dev[ts ostride + 2 i ..]; chunks of LAPH_NV vectors
static int enqueue_dots(const Launch &L, tmhip_cvfield *const *v, int nv, const tmhip_cvfield *x, double *out_dev, int ostride, const Mask &mask) {
  const dim3 g = stream_grid(L.g, L.nt);
  for (int first = 0; first < nv; first += LAPH_NV) {
    const int n = std::min(nv - first, LAPH_NV);
    Vecs V;
    memset(&V, 0, sizeof(V));
    for (int i = 0; i < n; i++) V.v[i] = v[first + i]->d;
    hipLaunchKernelGGL(laph_dots_kernel, g, dim3(LA_BS), 0, L.ctx->stream, V, n, (const v2d *)x->d, L.g, L.t0, mask, L.w->partials);
    hipLaunchKernelGGL(laph_final_kernel, dim3(2 * n, L.nt), dim3(256), 0, L.ctx->stream, (const double *)L.w->partials, (int)(g.x * g.y), 2 * n, out_dev + 2 * first, ostride, mask);
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
// x -= sum_i h_i v_i with h of slice ts at h_dev[ts hstride ..]; |x|^2 of slice ts -> n_dev[ts nstride]
static int enqueue_project(const Launch &L, tmhip_cvfield *const *v, int nv, tmhip_cvfield *x, const double *h_dev, int hstride, double *n_dev, int nstride, const Mask &mask) {
  const dim3 g = stream_grid(L.g, L.nt);
  int first = 0;
  do {
    const int n = std::min(nv - first, LAPH_NV);
    Vecs V;
    memset(&V, 0, sizeof(V));
    for (int i = 0; i < n; i++) V.v[i] = v[first + i]->d;
    hipLaunchKernelGGL(laph_project_kernel, g, dim3(LA_BS), 0, L.ctx->stream, V, n, x->d, h_dev + 2 * first, hstride, L.g, L.t0, mask, L.w->partials);
    first += n;
  } while (first < nv);
  hipLaunchKernelGGL(laph_final_kernel, dim3(1, L.nt), dim3(256), 0, L.ctx->stream, (const double *)L.w->partials, (int)(g.x * g.y), 1, n_dev, nstride, mask);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int enqueue_scale(const Launch &L, tmhip_cvfield *out, const tmhip_cvfield *in, const double *n_dev, int nstride, const Mask &mask) {
  hipLaunchKernelGGL(laph_scale_kernel, stream_grid(L.g, L.nt), dim3(LA_BS), 0, L.ctx->stream, out->d, (const v2d *)in->d, n_dev, nstride, L.g, L.t0, mask);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int enqueue_copy(const Launch &L, tmhip_cvfield *out, const tmhip_cvfield *in, const Mask &mask) {
  if (out->d == in->d) return 0;
  hipLaunchKernelGGL(laph_comb_kernel, stream_grid(L.g, L.nt), dim3(LA_BS), 0, L.ctx->stream, out->d, (const v2d *)nullptr, (const v2d *)in->d, (const v2d *)nullptr,
                     (const double *)nullptr, L.g, L.t0, mask);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
// Y: [nt][n][k] on the host
static int enqueue_rotate(const Launch &L, tmhip_cvfield *const *v, int n, int k, const double *Y, const Mask &mask) {
  const int KP = (k + LAPH_RG - 1) / LAPH_RG * LAPH_RG;
  std::vector<double> y((size_t)L.nt * n * KP, 0.0);
  for (int t = 0; t < L.nt; t++)
    for (int i = 0; i < n; i++)
      for (int c = 0; c < k; c++) y[((size_t)t * n + i) * KP + c] = Y[((size_t)t * n + i) * k + c];
  if (buffers(L.ctx, L.w, 0, y.size())) return 1;
  // the host arrives here with a new Y after a synchronisation (a cycle ends with one), so the buffer is free; the copy is waited for
  // because y goes out of scope
  TMHIP_CHECK(hipMemcpyAsync(L.w->y_dev, y.data(), y.size() * sizeof(double), hipMemcpyHostToDevice, L.ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(L.ctx->stream));
  Basis b;
  memset(&b, 0, sizeof(b));
  for (int i = 0; i < n; i++) b.v[i] = v[i]->d;
  const dim3 g((2 * L.g.S3 + 63) / 64, 3, L.nt);
  hipLaunchKernelGGL(laph_rotate_kernel, g, dim3(64), (size_t)n * 64 * sizeof(double), L.ctx->stream, b, n, k, (const double *)L.w->y_dev, KP, L.g, L.t0, mask);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

// ---- the driver -----------------------------------------------------------------------------------------------------------------
// One slice's side of the run: what lanczos() of eig.hip keeps in its locals
struct Slice {
  bool in_group, active, stepping, broke, capped, fresh, cycle, check, last, est_ok, need_res;
  int k, len, keep, keep_rule, got, conv, apps, failed;
  double beta, anorm, lo, hi;
  std::vector<double> T, S, th, theta, res, ritz, rres;
};

struct Call {
  Launch L;
  int m, nev, fused, max_apps, rs;   // rs: doubles of results per slice on the device
  double prec;
  std::vector<Slice> s;
  // the result block of slice ts at res_dev[ts rs ..]: h of the first pass [0, 2 nb), of the second [2 nb, 4 nb), n1, n2, then the
  // Rayleigh quotients (re, im) [nev] and the squared residual norms [nev] of a check
  int nb() const { return m + 1; }
  int off_n() const { return 4 * nb(); }
  int off_rq() const { return 4 * nb() + 2; }
  int off_rn() const { return 4 * nb() + 2 + 2 * nev; }
};

template <class Pred>
static Mask mask_where(const Call &c, Pred p) {
  Mask m;
  memset(&m, 0, sizeof(m));
  for (int i = 0; i < c.L.nt; i++) if (p(c.s[i])) m.w[i >> 6] |= 1ull << (i & 63);
  return m;
}

static int fetch(Call &c) {
  Work *w = c.L.w;
  TMHIP_CHECK(hipMemcpyAsync(w->res_host, w->res_dev, (size_t)c.L.nt * c.rs * sizeof(double), hipMemcpyDeviceToHost, c.L.ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(c.L.ctx->stream));
  return 0;
}

// the coefficients of the Chebyshev steps of every slice: table 0 = the first step (a, c, -), table 1 = the others (2 a, 2 c, -1)
static int upload_coef(Call &c) {
  std::vector<double> t((size_t)2 * c.L.nt * 3, 0.0);
  for (int i = 0; i < c.L.nt; i++) {
    const Slice &s = c.s[i];
    if (!(s.hi > s.lo)) continue;
    const double a = -2.0 / (s.hi - s.lo), cc = (s.hi + s.lo) / (s.hi - s.lo);
    t[3 * i] = a; t[3 * i + 1] = cc;
    t[(size_t)3 * (c.L.nt + i)] = 2.0 * a; t[(size_t)3 * (c.L.nt + i) + 1] = 2.0 * cc; t[(size_t)3 * (c.L.nt + i) + 2] = -1.0;
  }
  TMHIP_CHECK(hipMemcpyAsync(c.L.w->coef_dev, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, c.L.ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(c.L.ctx->stream));
  return 0;
}

// out = B in for the slices of `mask`, B = A (deg 0) or T_deg((hi + lo - 2 A) / (hi - lo)) with the interval of each slice; `out` is
// one of the three buffers and may not be `in`.  Nothing but launches: no synchronisation inside the filter.
static int apply_filtered(Call &c, int deg, tmhip_cvfield *out, tmhip_cvfield *in, tmhip_cvfield *w0, tmhip_cvfield *w1, const Mask &mask) {
  if (deg <= 0) return enqueue_apply(c.L, c.fused, 0, out->d, in->d, nullptr, nullptr, nullptr, 0, mask);
  tmhip_cvfield *buf[3] = {out, w0, w1};   // t_k lives in buf[(deg - k) % 3]: t_deg in `out`
  tmhip_cvfield *tprev = nullptr, *tcur = in;
  for (int k = 1; k <= deg; k++) {
    tmhip_cvfield *tn = buf[(deg - k) % 3];
    if (enqueue_apply(c.L, c.fused, 2, tn->d, tcur->d, k == 1 ? nullptr : tprev->d, c.L.w->coef_dev + (k == 1 ? 0 : (size_t)3 * c.L.nt), nullptr, 0, mask)) return 1;
    tprev = tcur; tcur = tn;
  }
  return 0;
}

// theta_i = <v_i, A v_i> and |A v_i - theta_i v_i| of the unit vectors v[0 .. got) of the slices marked need_res: one application each
// with the Rayleigh quotient from the same pass, the residual through the projection with it as the coefficient; all of them enqueued,
// ONE synchronisation
static int true_residuals(Call &c) {
  Work *w = c.L.w;
  int most = 0;
  for (Slice &s : c.s) if (s.need_res) most = std::max(most, s.got);
  if (!most) return 0;
  tmhip_cvfield *w0 = w->v[c.m + 1];
  for (int i = 0; i < most; i++) {
    const Mask mask = mask_where(c, [&](const Slice &s) { return s.need_res && i < s.got; });
    if (enqueue_apply(c.L, c.fused, 1, w0->d, w->v[i]->d, nullptr, nullptr, w->res_dev + c.off_rq() + 2 * i, c.rs, mask)) return 1;
    if (enqueue_project(c.L, &w->v[i], 1, w0, w->res_dev + c.off_rq() + 2 * i, c.rs, w->res_dev + c.off_rn() + i, c.rs, mask)) return 1;
  }
  if (fetch(c)) return 1;
  for (int t = 0; t < c.L.nt; t++) {
    Slice &s = c.s[t];
    if (!s.need_res) continue;
    const double *r = w->res_host + (size_t)t * c.rs;
    s.conv = 0;
    for (int i = 0; i < s.got; i++) {
      s.theta[i] = r[c.off_rq() + 2 * i];
      s.res[i] = sqrt(r[c.off_rn() + i]);
      if (s.res[i] <= c.prec) s.conv++;
    }
    s.apps += s.got;
    s.fresh = true;
    s.need_res = false;
  }
  return 0;
}

// the small eigenproblems of the slices marked `cycle`, on up to LAPH_HOST_THREADS host threads
static void small_problems(Call &c) {
  const auto begin = std::chrono::steady_clock::now();
  struct Clock { Work *w; std::chrono::steady_clock::time_point b; ~Clock() { w->small_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - b).count(); } } clock = {c.L.w, begin};
  std::vector<int> todo;
  for (int t = 0; t < c.L.nt; t++) if (c.s[t].cycle) todo.push_back(t);
  auto solve = [&](int first, int step) {
    for (size_t q = first; q < todo.size(); q += step) {
      Slice &s = c.s[todo[q]];
      const int len = s.len, m = c.m;
      s.S.assign((size_t)len * len, 0.0);
      s.th.assign(len, 0.0);
      for (int i = 0; i < len; i++) for (int j = 0; j < len; j++) s.S[(size_t)i * len + j] = s.T[(size_t)i * m + j];
      s.failed = tmhip_eig_small_jacobi(len, s.S.data(), s.th.data());
    }
  };
  const int nth = (int)std::min<size_t>(LAPH_HOST_THREADS, todo.size());
  if (nth <= 1) { solve(0, 1); return; }
  std::vector<std::thread> th;
  for (int i = 1; i < nth; i++) th.emplace_back(solve, i, nth);
  solve(0, nth);
  for (std::thread &x : th) x.join();
}

// One thick-restart Lanczos run on B = filter(A) for the slices marked in_group, all with the same degree, from the unit start vectors
// in v[0].  The statements of lanczos() of eig.hip per slice; the loops over cycles and steps are shared: every launch serves the slices
// that are at that statement, a slice that leaves a cycle early (its cap, an invariant subspace) or ends its run is masked out.
static int lanczos(Call &c, bool largest, int deg, bool one_cycle) {
  Work *w = c.L.w;
  tmhip_cvfield **v = w->v.data();
  const int m = c.m, nev = c.nev, nb = c.nb();
  tmhip_cvfield *w0 = v[m + 1], *w1 = v[m + 2];
  const int step_cost = deg > 0 ? deg : 1;
  for (Slice &s : c.s) {
    s.active = s.in_group;
    s.k = 0; s.fresh = false; s.anorm = 0.0; s.conv = 0; s.got = 0; s.need_res = false;
    s.T.assign((size_t)m * m, 0.0);
    s.ritz.clear(); s.rres.clear(); s.keep_rule = 0;
  }
  int k = 0;   // of every active slice: a slice that goes on has run a whole cycle, so all of them keep the same number
  for (;;) {
    for (Slice &s : c.s) { s.stepping = s.active; s.len = s.k; s.broke = s.capped = s.cycle = false; s.beta = 0.0; }
    for (int j = k; j < m; j++) {
      for (Slice &s : c.s)
        if (s.stepping && s.apps + step_cost + nev > c.max_apps) { s.capped = true; s.stepping = false; }
      const Mask mask = mask_where(c, [](const Slice &s) { return s.stepping; });
      if (!mask_any(mask)) break;
      if (apply_filtered(c, deg, v[j + 1], v[j], w0, w1, mask)) return 1;
      // classical Gram-Schmidt, twice, and the scaling: nine launches (more when the basis takes chunks), ONE copy and synchronisation
      double *r = w->res_dev;
      if (enqueue_dots(c.L, v, j + 1, v[j + 1], r, c.rs, mask) || enqueue_project(c.L, v, j + 1, v[j + 1], r, c.rs, r + c.off_n(), c.rs, mask)) return 1;
      if (enqueue_dots(c.L, v, j + 1, v[j + 1], r + 2 * nb, c.rs, mask) || enqueue_project(c.L, v, j + 1, v[j + 1], r + 2 * nb, c.rs, r + c.off_n() + 1, c.rs, mask)) return 1;
      if (enqueue_scale(c.L, v[j + 1], v[j + 1], r + c.off_n() + 1, c.rs, mask)) return 1;
      if (fetch(c)) return 1;
      for (int t = 0; t < c.L.nt; t++) {
        Slice &s = c.s[t];
        if (!s.stepping) continue;
        const double *h1 = w->res_host + (size_t)t * c.rs, *h2 = h1 + 2 * nb;
        const double n2 = h1[c.off_n() + 1];
        s.apps += step_cost;
        s.T[(size_t)j * m + j] = h1[2 * j] + h2[2 * j];
        s.beta = sqrt(n2);
        double before = n2;
        for (int i = 0; i <= j; i++) { const double re = h1[2 * i] + h2[2 * i], im = h1[2 * i + 1] + h2[2 * i + 1]; before += re * re + im * im; }
        s.anorm = std::max(s.anorm, sqrt(before));
        s.len = j + 1;
        if (!(s.beta > 1e-14 * s.anorm)) { s.broke = true; s.beta = 0.0; s.stepping = false; continue; }   // an invariant subspace: the cycle ends at this length
        if (j + 1 < m) s.T[(size_t)j * m + j + 1] = s.T[(size_t)(j + 1) * m + j] = s.beta;
      }
    }
    // the end of the cycle, slice by slice
    for (Slice &s : c.s) {
      if (!s.active) continue;
      if (s.len == s.k && s.capped) {
        // no room for another step: what the last restart kept (or the start vector alone) is the answer
        s.got = std::min(nev, std::max(s.k, 1));
        s.active = false;
        if (!one_cycle && !s.fresh) s.need_res = true;
        continue;
      }
      s.cycle = true;
    }
    small_problems(c);
    int nmax = 0, kmax = 0;
    for (Slice &s : c.s) {
      if (!s.cycle) continue;
      if (s.failed) TMHIP_FAIL("laph_eigensystem: the projected eigenproblem did not converge");
      const int len = s.len;
      if (one_cycle) {
        s.ritz.assign(s.th.begin(), s.th.begin() + len);
        s.rres.resize(len);
        for (int i = 0; i < len; i++) s.rres[i] = fabs(s.beta * s.S[(size_t)(len - 1) * len + i]);
      }
      // how many Ritz vectors the restart keeps: nev + (m - nev) / 2, capped at m - 2 and by what the cycle has
      int keep = nev + (m - nev) / 2;
      if (keep > m - 2) keep = m - 2;
      if (keep > len - 1) keep = len - 1;
      if (keep < 1) keep = 1;
      s.keep_rule = keep;
      s.last = s.broke || s.capped || one_cycle;
      if (s.last && keep < std::min(nev, len)) keep = std::min(nev, len);
      s.keep = keep;
      nmax = std::max(nmax, len); kmax = std::max(kmax, keep);
    }
    if (nmax) {
      // one rotation for all: Y of a slice with a shorter cycle or fewer kept vectors is padded with zeros (such a slice ends here)
      auto col = [&](const Slice &s, int i) { return largest ? s.len - 1 - i : i; };
      std::vector<double> Y((size_t)c.L.nt * nmax * kmax, 0.0);
      for (int t = 0; t < c.L.nt; t++) {
        Slice &s = c.s[t];
        if (!s.cycle) continue;
        const int len = s.len;
        for (int i = 0; i < len; i++) for (int q = 0; q < s.keep; q++) Y[((size_t)t * nmax + i) * kmax + q] = s.S[(size_t)i * len + col(s, q)];
        s.est_ok = true;
        for (int q = 0; q < std::min(nev, s.keep); q++) s.est_ok = s.est_ok && fabs(s.beta * s.S[(size_t)(len - 1) * len + col(s, q)]) <= c.prec;
        s.got = std::min(nev, s.keep);
        s.check = (s.last || deg > 0 || s.est_ok) && !one_cycle;
        if (s.check) s.need_res = true; else s.fresh = false;
      }
      if (enqueue_rotate(c.L, v, nmax, kmax, Y.data(), mask_where(c, [](const Slice &s) { return s.cycle; }))) return 1;
    }
    if (true_residuals(c)) return 1;
    bool go_on = false;
    for (Slice &s : c.s) {
      if (!s.cycle) continue;
      if (one_cycle || s.last || (s.check && s.conv == nev)) { s.active = false; continue; }
      go_on = true;
    }
    if (!go_on) return 0;
    // restart: v[keep] = the residual vector, T = diag(theta) with the arrow beta s_{len-1, i}
    int keep = 0;
    for (Slice &s : c.s) if (s.active) keep = s.keep;
    if (enqueue_copy(c.L, v[keep], v[m], mask_where(c, [](const Slice &s) { return s.active; }))) return 1;
    for (Slice &s : c.s) {
      if (!s.active) continue;
      const int len = s.len;
      std::fill(s.T.begin(), s.T.end(), 0.0);
      for (int q = 0; q < keep; q++) {
        const int cq = largest ? len - 1 - q : q;
        s.T[(size_t)q * m + q] = s.th[cq];
        s.T[(size_t)q * m + keep] = s.T[(size_t)keep * m + q] = s.beta * s.S[(size_t)(len - 1) * len + cq];
      }
      s.k = keep;
    }
    k = keep;
  }
}

static int run(tmhip_ctx *ctx, int t0, int nt, int nev, double prec, int max_apps, tmhip_cvfield *const *evec, double *evals, double *resid, int *converged, int *apps) {
  const char *who = "laph_eigensystem";
  if (with_links(ctx, who) || range_ok(ctx, who, t0, nt)) return 1;
  if (!evals || !resid || !converged || !apps) TMHIP_FAIL("%s: null argument", who);
  const int m = ctx->opt_laph_basis ? ctx->opt_laph_basis : std::min(nev + 32, TMHIP_LAPH_MAX_BASIS);
  if (nev < 1 || nev + 2 > m) TMHIP_FAIL("%s: nev = %d needs nev >= 1 and nev + 2 <= laph_basis = %d", who, nev, m);
  if (!(prec > 0.0)) TMHIP_FAIL("%s: prec must be positive", who);
  if (max_apps < nev + 1) TMHIP_FAIL("%s: max_apps = %d is too small for nev = %d (at least nev + 1)", who, max_apps, nev);
  if (evec)
    for (int i = 0; i < nev; i++) {
      char name[32];
      snprintf(name, sizeof(name), "evec[%d]", i);
      if (field_ok(ctx, who, evec[i], name)) return 1;
      for (int j = 0; j < i; j++) if (evec[j]->d == evec[i]->d) TMHIP_FAIL("%s: evec[%d] is evec[%d]", who, i, j);
    }
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  Call c;
  c.L.ctx = ctx; c.L.w = w; c.L.g = geom_of(ctx); c.L.t0 = t0; c.L.nt = nt;
  c.m = m; c.nev = nev; c.fused = ctx->opt_laph_fused; c.max_apps = max_apps; c.prec = prec;
  c.rs = 4 * (m + 1) + 2 + 3 * nev;
  if (buffers(ctx, w, (size_t)nt * c.rs, 0) || reserve(ctx, w, m + 3)) return 1;
  c.s.resize(nt);
  for (Slice &s : c.s) { s.apps = 0; s.lo = w->lo; s.hi = w->hi; s.in_group = true; s.theta.assign(nev, 0.0); s.res.assign(nev, 0.0); s.failed = 0; s.need_res = false; s.got = 0; s.conv = 0; }
  tmhip_cvfield **v = w->v.data();
  const Mask all = mask_all(nt);
  double *nrm = w->res_dev + c.off_n();
  // the start vectors: evec[0] where its norm is non-zero, else the fixed pseudo-random fill
  Mask fill = all;
  if (evec) {
    if (enqueue_copy(c.L, v[m + 1], evec[0], all) || enqueue_project(c.L, nullptr, 0, v[m + 1], w->res_dev, c.rs, nrm, c.rs, all) || enqueue_scale(c.L, v[0], v[m + 1], nrm, c.rs, all)) return 1;
    if (fetch(c)) return 1;
    memset(&fill, 0, sizeof(fill));
    for (int t = 0; t < nt; t++) {
      const double n2 = w->res_host[(size_t)t * c.rs + c.off_n()];
      if (!(n2 > 0.0 && std::isfinite(n2))) fill.w[t >> 6] |= 1ull << (t & 63);
    }
  }
  if (mask_any(fill)) {
    hipLaunchKernelGGL(laph_fill_kernel, dim3((c.L.g.S3 + LA_BS - 1) / LA_BS, 3, nt), dim3(LA_BS), 0, ctx->stream, v[m + 1]->d, c.L.g, t0, fill);
    TMHIP_CHECK(hipGetLastError());
    if (enqueue_project(c.L, nullptr, 0, v[m + 1], w->res_dev, c.rs, nrm, c.rs, fill) || enqueue_scale(c.L, v[0], v[m + 1], nrm, c.rs, fill)) return 1;
  }
  const int deg = ctx->opt_laph_cheb;
  if (deg > 0) {
    // the interval of every slice that has none from one unfiltered cycle: hi = 1.1 (largest Ritz value + its residual bound); lo = the
    // largest Ritz value the restart rule would keep
    bool any = false;
    for (Slice &s : c.s) { s.in_group = !(s.hi > s.lo); any = any || s.in_group; }
    if (any) {
      if (lanczos(c, false, 0, true)) return 1;
      for (Slice &s : c.s) {
        if (!s.in_group) continue;
        const int len = (int)s.ritz.size();
        if (len >= nev + 2) {
          s.hi = 1.1 * (s.ritz[len - 1] + s.rres[len - 1]);
          s.lo = s.ritz[std::min(s.keep_rule, len) - 1];
        }
        // a cycle the cap cut short (or did not allow at all), or an invariant subspace smaller than the basis: nothing to filter, run plain
        if (!(s.hi > s.lo) || len < nev + 2) { s.lo = s.hi = 0.0; s.in_group = false; }
      }
      // the filtered run starts from the sum of the nev lowest Ritz vectors, v[0 .. nev) after the cycle's rotation
      const Mask summed = mask_where(c, [](const Slice &s) { return s.in_group; });
      if (mask_any(summed)) {
        std::vector<double> y((size_t)nt * nev, 1.0 / sqrt((double)nev));
        if (enqueue_rotate(c.L, v, nev, 1, y.data(), summed)) return 1;
      }
    }
  }
  // the slices with an interval run filtered, the others plain: two groups, one after the other (the second is empty as a rule)
  for (int pass = 0; pass < 2; pass++) {
    const bool filtered = pass == 0;
    bool any = false;
    for (Slice &s : c.s) { s.in_group = (deg > 0 && s.hi > s.lo) == filtered; any = any || s.in_group; }
    if (!any) continue;
    if (filtered && upload_coef(c)) return 1;
    if (lanczos(c, filtered, filtered ? deg : 0, false)) return 1;
  }
  // ascending; the vectors follow: a permutation per slice, done as a rotation, then the copies
  int most = 0;
  for (Slice &s : c.s) most = std::max(most, s.got);
  std::vector<double> P((size_t)nt * most * most, 0.0);
  for (int t = 0; t < nt; t++) {
    Slice &s = c.s[t];
    std::vector<int> order(s.got);
    for (int i = 0; i < s.got; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return s.theta[a] < s.theta[b]; });
    for (int i = 0; i < nev; i++) {
      if (i < s.got) { evals[(size_t)t * nev + i] = s.theta[order[i]]; resid[(size_t)t * nev + i] = s.res[order[i]]; }
      else { evals[(size_t)t * nev + i] = s.theta[order[s.got - 1]]; resid[(size_t)t * nev + i] = HUGE_VAL; }   // fewer vectors than nev: never counted as converged
    }
    for (int i = 0; i < most; i++) P[((size_t)t * most + (i < s.got ? order[i] : i)) * most + i] = 1.0;
    converged[t] = s.conv;
    apps[t] = s.apps;
  }
  if (evec) {
    if (enqueue_rotate(c.L, v, most, most, P.data(), all)) return 1;
    for (int i = 0; i < most; i++)
      if (enqueue_copy(c.L, evec[i], v[i], mask_where(c, [&](const Slice &s) { return i < s.got; }))) return 1;
  }
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace laphhip
using namespace laphhip;

void tmhip_laph_destroy(tmhip_ctx *ctx) { laphhip::destroy(ctx); }

extern "C" {

int tmhip_cvfield_alloc(tmhip_ctx *ctx, tmhip_cvfield **out) {
  if (!out) TMHIP_FAIL("tmhip_cvfield_alloc: null argument");
  if (unsplit(ctx, "tmhip_cvfield_alloc")) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  tmhip_cvfield *f = new (std::nothrow) tmhip_cvfield();
  if (!f) TMHIP_FAIL("out of host memory");
  f->ctx = ctx; f->cs = geom_of(ctx).cs; f->d = nullptr;
  const size_t bytes = (size_t)3 * f->cs * sizeof(v2d);
  if (hipMalloc((void **)&f->d, bytes) != hipSuccess) { delete f; TMHIP_FAIL("tmhip_cvfield_alloc: out of device memory"); }
  TMHIP_CHECK(hipMemsetAsync(f->d, 0, bytes, ctx->stream));
  *out = f;
  return 0;
}

void tmhip_cvfield_free(tmhip_ctx *ctx, tmhip_cvfield *f) {
  (void)ctx;
  if (!f) return;
  if (f->d) (void)hipFree(f->d);
  delete f;
}

int tmhip_cvfield_zero(tmhip_ctx *ctx, tmhip_cvfield *f) {
  if (unsplit(ctx, "tmhip_cvfield_zero") || field_ok(ctx, "tmhip_cvfield_zero", f, "the field")) return 1;
  TMHIP_CHECK(hipMemsetAsync(f->d, 0, (size_t)3 * f->cs * sizeof(v2d), ctx->stream));
  return 0;
}

int tmhip_cvfield_upload_slices(tmhip_ctx *ctx, tmhip_cvfield *f, const void *host, int t0, int nt) {
  if (unsplit(ctx, "tmhip_cvfield_upload") || field_ok(ctx, "tmhip_cvfield_upload", f, "the field") || slices_ok(ctx, "tmhip_cvfield_upload", t0, nt)) return 1;
  if (!host) TMHIP_FAIL("tmhip_cvfield_upload: null argument");
  const int S3 = geom_of(ctx).S3, n = nt * S3;
  const size_t bytes = (size_t)n * 3 * sizeof(v2d);
  if (tmhip_stage_reserve(ctx, bytes)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(ctx->stage, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(cv_layout_kernel<true>, dim3((3 * n + 255) / 256), dim3(256), 0, ctx->stream, (v2d *)ctx->stage, f->d + (size_t)t0 * S3, f->cs, n);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));   // the staging buffer is reused by the next call
  return 0;
}

int tmhip_cvfield_download_slices(tmhip_ctx *ctx, tmhip_cvfield *f, void *host, int t0, int nt) {
  if (unsplit(ctx, "tmhip_cvfield_download") || field_ok(ctx, "tmhip_cvfield_download", f, "the field") || slices_ok(ctx, "tmhip_cvfield_download", t0, nt)) return 1;
  if (!host) TMHIP_FAIL("tmhip_cvfield_download: null argument");
  const int S3 = geom_of(ctx).S3, n = nt * S3;
  const size_t bytes = (size_t)n * 3 * sizeof(v2d);
  if (tmhip_stage_reserve(ctx, bytes)) return 1;
  hipLaunchKernelGGL(cv_layout_kernel<false>, dim3((3 * n + 255) / 256), dim3(256), 0, ctx->stream, (v2d *)ctx->stage, f->d + (size_t)t0 * S3, f->cs, n);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(host, ctx->stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tmhip_cvfield_upload(tmhip_ctx *ctx, tmhip_cvfield *f, const void *host) { return tmhip_cvfield_upload_slices(ctx, f, host, 0, ctx ? ctx->g.T : 0); }
int tmhip_cvfield_download(tmhip_ctx *ctx, tmhip_cvfield *f, void *host) { return tmhip_cvfield_download_slices(ctx, f, host, 0, ctx ? ctx->g.T : 0); }

static int apply_entry(tmhip_ctx *ctx, const char *who, int mode, tmhip_cvfield *out, tmhip_cvfield *in, tmhip_cvfield *prev, int t0, int nt, const double *coef, double *dots) {
  if (with_links(ctx, who) || range_ok(ctx, who, t0, nt) || field_ok(ctx, who, out, "out") || field_ok(ctx, who, in, "in")) return 1;
  if (prev && field_ok(ctx, who, prev, "prev")) return 1;
  if (out->d == in->d) TMHIP_FAIL("%s: out == in (other threads of the launch read the neighbours of a site)", who);
  if (prev && out->d == prev->d) TMHIP_FAIL("%s: out == prev", who);
  if ((mode == 1 && !dots) || (mode == 2 && !coef)) TMHIP_FAIL("%s: null argument", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  if (buffers(ctx, w, (size_t)3 * nt, 0)) return 1;
  Launch L = {ctx, w, geom_of(ctx), t0, nt};
  if (mode == 2) {
    TMHIP_CHECK(hipMemcpyAsync(w->res_dev, coef, (size_t)3 * nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (enqueue_apply(L, ctx->opt_laph_fused, mode, out->d, in->d, prev ? prev->d : nullptr, w->res_dev, w->res_dev, 2, mask_all(nt))) return 1;
  if (mode == 1) {
    TMHIP_CHECK(hipMemcpyAsync(w->res_host, w->res_dev, (size_t)2 * nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(dots, w->res_host, (size_t)2 * nt * sizeof(double));
  }
  return 0;
}

int tmhip_laph_apply(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt) {
  return apply_entry(ctx, "laph_apply", 0, out, in, nullptr, t0, nt, nullptr, nullptr);
}
int tmhip_laph_apply_dot(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt, double *dots) {
  return apply_entry(ctx, "laph_apply_dot", 1, out, in, nullptr, t0, nt, nullptr, dots);
}
int tmhip_laph_apply_filter(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, tmhip_cvfield *prev, int t0, int nt, const double *coef) {
  return apply_entry(ctx, "laph_apply_filter", 2, out, in, prev, t0, nt, coef, nullptr);
}

// the checks the pieces share; the results of a piece: `res` doubles
static int piece_entry(tmhip_ctx *ctx, const char *who, int nv, int most, tmhip_cvfield *const *v, tmhip_cvfield *w, int t0, int nt, size_t res, size_t ylen, Launch *L) {
  if (unsplit(ctx, who) || range_ok(ctx, who, t0, nt)) return 1;
  if (nv < 0 || nv > most) TMHIP_FAIL("%s: %d vectors, at most %d", who, nv, most);
  if (nv && !v) TMHIP_FAIL("%s: null argument", who);
  if (w && field_ok(ctx, who, w, "w")) return 1;
  for (int i = 0; i < nv; i++) {
    char name[32];
    snprintf(name, sizeof(name), "v[%d]", i);
    if (field_ok(ctx, who, v[i], name)) return 1;
  }
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *wk = work_of(ctx);
  if (buffers(ctx, wk, res, ylen)) return 1;
  L->ctx = ctx; L->w = wk; L->g = geom_of(ctx); L->t0 = t0; L->nt = nt;
  return 0;
}

int tmhip_laph_dots(tmhip_ctx *ctx, int nv, tmhip_cvfield *const *v, tmhip_cvfield *w, int t0, int nt, const int *active, double *out) {
  Launch L;
  if (!out || !w || nv < 1) TMHIP_FAIL("laph_dots: null argument or no vectors");
  if (piece_entry(ctx, "laph_dots", nv, LAPH_NB, v, w, t0, nt, (size_t)2 * nv * nt, 0, &L)) return 1;
  const Mask mask = mask_from(active, nt);
  if (enqueue_dots(L, v, nv, w, L.w->res_dev, 2 * nv, mask)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(L.w->res_host, L.w->res_dev, (size_t)2 * nv * nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int t = 0; t < nt; t++) if (mask.on(t)) memcpy(out + (size_t)2 * nv * t, L.w->res_host + (size_t)2 * nv * t, (size_t)2 * nv * sizeof(double));
  return 0;
}

int tmhip_laph_project(tmhip_ctx *ctx, int nv, tmhip_cvfield *const *v, tmhip_cvfield *w, const double *h, int t0, int nt, const int *active, double *sqnorm) {
  Launch L;
  if (!sqnorm || !w || (nv && !h)) TMHIP_FAIL("laph_project: null argument");
  if (piece_entry(ctx, "laph_project", nv, LAPH_NB, v, w, t0, nt, (size_t)(2 * nv + 1) * nt, 0, &L)) return 1;
  for (int i = 0; i < nv; i++) if (v[i]->d == w->d) TMHIP_FAIL("laph_project: w is v[%d] (other blocks of the launch read it)", i);
  const Mask mask = mask_from(active, nt);
  double *n_dev = L.w->res_dev + (size_t)2 * nv * nt;
  if (nv) {
    TMHIP_CHECK(hipMemcpyAsync(L.w->res_dev, h, (size_t)2 * nv * nt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (enqueue_project(L, v, nv, w, L.w->res_dev, 2 * nv, n_dev, 1, mask)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(L.w->res_host, n_dev, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int t = 0; t < nt; t++) if (mask.on(t)) sqnorm[t] = L.w->res_host[t];
  return 0;
}

int tmhip_laph_normalise(tmhip_ctx *ctx, tmhip_cvfield *out, tmhip_cvfield *in, int t0, int nt, const int *active, double *sqnorm) {
  Launch L;
  if (!sqnorm || !in) TMHIP_FAIL("laph_normalise: null argument");
  if (piece_entry(ctx, "laph_normalise", 0, 0, nullptr, in, t0, nt, (size_t)nt, 0, &L) || field_ok(ctx, "laph_normalise", out, "out")) return 1;
  const Mask mask = mask_from(active, nt);
  if (enqueue_project(L, nullptr, 0, in, L.w->res_dev, 0, L.w->res_dev, 1, mask) || enqueue_scale(L, out, in, L.w->res_dev, 1, mask)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(L.w->res_host, L.w->res_dev, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int t = 0; t < nt; t++) if (mask.on(t)) sqnorm[t] = L.w->res_host[t];
  return 0;
}

int tmhip_laph_rotate(tmhip_ctx *ctx, int n, int k, tmhip_cvfield *const *v, const double *Y, int t0, int nt, const int *active) {
  Launch L;
  if (n < 1 || n > TMHIP_LAPH_MAX_BASIS || k < 1 || k > n) TMHIP_FAIL("laph_rotate: n = %d, k = %d, needs 1 <= k <= n <= %d", n, k, TMHIP_LAPH_MAX_BASIS);
  if (!Y) TMHIP_FAIL("laph_rotate: null argument");
  if (piece_entry(ctx, "laph_rotate", n, TMHIP_LAPH_MAX_BASIS, v, nullptr, t0, nt, 0, 0, &L)) return 1;
  for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (v[i]->d == v[j]->d) TMHIP_FAIL("laph_rotate: v[%d] is v[%d]", i, j);
  if (enqueue_rotate(L, v, n, k, Y, mask_from(active, nt))) return 1;
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tmhip_laph_set_interval(tmhip_ctx *ctx, double lo, double hi) {
  if (!ctx) TMHIP_FAIL("laph_set_interval: null context");
  if (!(lo == 0.0 && hi == 0.0) && !(hi > lo && lo > 0.0)) TMHIP_FAIL("laph_set_interval: needs 0 < lo < hi, or 0, 0 for the automatic interval");
  Work *w = work_of(ctx);
  w->lo = lo; w->hi = hi;
  return 0;
}

int tmhip_laph_eigensystem(tmhip_ctx *ctx, int t0, int nt, int nev, double prec, int max_apps, tmhip_cvfield *const *evec, double *evals, double *resid, int *converged,
                           int *apps) {
  const auto begin = std::chrono::steady_clock::now();
  if (ctx && ctx->laph) ((Work *)ctx->laph)->small_s = 0.0;
  const int rc = laphhip::run(ctx, t0, nt, nev, prec, max_apps, evec, evals, resid, converged, apps);
  if (ctx && ctx->laph) ((Work *)ctx->laph)->total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
  return rc;
}

int tmhip_laph_timing(tmhip_ctx *ctx, double out[2]) {
  if (!ctx || !out) TMHIP_FAIL("laph_timing: null argument");
  Work *w = work_of(ctx);
  out[0] = w->small_s; out[1] = w->total_s;
  return 0;
}

int tmhip_laph_write(tmhip_ctx *ctx, const char *dir, int nstore, int t0, int nt, int nev, tmhip_cvfield *const *evec, const double *evals) {
  const char *who = "laph_write";
  if (unsplit(ctx, who) || range_ok(ctx, who, t0, nt)) return 1;
  if (!dir || !evec || !evals || nev < 1) TMHIP_FAIL("%s: null argument", who);
  for (int i = 0; i < nev; i++) if (field_ok(ctx, who, evec[i], "an eigenvector")) return 1;
  const size_t S3 = (size_t)ctx->g.LX * ctx->g.LY * ctx->g.LZ;
  std::vector<double> host((size_t)ctx->V * 6);
  char path[1024];
  // eigenvalues_Jacobi.c:176-209, the branch without MPI
  for (int t = t0; t < t0 + nt; t++) {
    snprintf(path, sizeof(path), "%s/eigenvalues.%.3d.%.4d", dir, t, nstore);
    FILE *f = fopen(path, "w");
    if (!f) TMHIP_FAIL("%s: cannot write %s", who, path);
    for (int i = 0; i < nev; i++) fprintf(f, "%e\n", evals[(size_t)(t - t0) * nev + i]);
    if (fclose(f)) TMHIP_FAIL("%s: error writing %s", who, path);
  }
  for (int i = 0; i < nev; i++) {
    if (tmhip_cvfield_download(ctx, evec[i], host.data())) return 1;
    for (int t = t0; t < t0 + nt; t++) {
      snprintf(path, sizeof(path), "%s/eigenvector.%.3d.%.3d.%.4d", dir, i, t, nstore);
      FILE *f = fopen(path, "wb");
      if (!f) TMHIP_FAIL("%s: cannot write %s", who, path);
      const size_t n = fwrite(host.data() + (size_t)t * S3 * 6, 6 * sizeof(double), S3, f);
      if (fclose(f) || n != S3) TMHIP_FAIL("%s: error writing %s", who, path);
    }
  }
  return 0;
}

}  // extern "C"
