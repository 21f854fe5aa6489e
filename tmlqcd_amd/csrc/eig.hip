// Eigenvalue measurement on the device (gfx950): thick-restart Lanczos (Wu and Simon) for the nev lowest or highest eigenpairs of a
// Hermitian positive operator of the operator table, with an optional Chebyshev filter for the lowest end.  It stands where the
// reference has solver/eigenvalues.c and solver/eigenvalues_bi.c over jdher / jdher_bi (Jacobi-Davidson on LAPACK with host vectors):
// here the basis, the work vectors and every coefficient of a step stay in HBM, the host sees one block of scalars per step.
//
// A "vector" is one or two SEGMENTS of `planes` SoA planes of n sites at stride ns: one EO field (12 planes), one FULL field (24
// planes: its odd half follows its even half at the same stride) or the doublet (up, dn) (two segments of 12).  Every kernel takes
// grid = (blocks of a plane, planes, segments), so one launch serves both flavours.
//
//   eig_dots_kernel      h_i = <v_i, w>, i < nv <= 65, in one pass: w once, every v_i once; per-thread order, block sum, partials
//                        layout and final pass are those of csg_dot_kernel<1> / reduce_final_multi_kernel (linalg.hip), so a value
//                        carries the bits of tmhip_scalar_prod of the same pair (two segments: the two totals, added up first)
//   eig_project_kernel   w -= sum_i h_i v_i, ascending i, h read from the device buffer the dots left; block sums of |w|^2 in the pass
//   eig_scale_kernel     out = w / sqrt(|w|^2), the norm read from the device
//   basis_rotate_kernel  V[:, 0:k] = V[:, 0:n] Y in place (the restart): a thread owns one complex element across all n vectors
//   eig_cheb_kernel      out = c1 x + c2 y + c3 z: the Chebyshev step t_next = 2 (a A t + c t) - t_prev beside the operator
#include "tmhip_internal.h"
#include "eig_small.h"
#include <vector>
#include <algorithm>

namespace eighip {

#define EIG_NV (TMHIP_EIG_MAX_BASIS + 1)
struct Basis { v2d *v[EIG_NV][2]; };
struct Pair { v2d *p[2]; };

__global__ __launch_bounds__(LA_BS, 8) void eig_dots_kernel(const Basis V, int nv, const Pair W, int ns, int n, double *partials) {
  __shared__ double wsum[2 * EIG_NV][LA_BS / 64];
  const int s = blockIdx.z;
  const size_t off = (size_t)blockIdx.y * ns;
  const v2d *w = W.p[s] + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
  v2d b[LA_UNROLL];
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) b[u] = base + u * LA_BS < n ? w[base + u * LA_BS] : v2d{0.0, 0.0};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = 0; i < nv; i++) {
    const v2d *vi = V.v[i][s] + off;
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
    partials[((size_t)s * 2 * nv + k) * per + blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// value k = blockIdx.x of nvals: the fixed-order pass of reduce_final_multi_kernel over the `per` block sums of each segment, the
// segments' totals added first to last
__global__ __launch_bounds__(256) void eig_final_kernel(const double *__restrict__ partials, int per, int nvals, int nseg, double *out) {
  __shared__ double sm[256];
  double total = 0.0;
  for (int s = 0; s < nseg; s++) {
    const double *p = partials + ((size_t)s * nvals + blockIdx.x) * per;
    double acc = 0.0;
    for (int i = threadIdx.x; i < per; i += 256) acc += p[i];
    __syncthreads();
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int q = 128; q > 0; q >>= 1) {
      if ((int)threadIdx.x < q) sm[threadIdx.x] += sm[threadIdx.x + q];
      __syncthreads();
    }
    total = s == 0 ? sm[0] : total + sm[0];
  }
  if (threadIdx.x == 0) out[blockIdx.x] = total;
}

__global__ __launch_bounds__(LA_BS, 8) void eig_project_kernel(const Basis V, int nv, const Pair W, const double *__restrict__ h, int ns, int n,
                                                               double *partials) {
  __shared__ double wsum[LA_BS / 64];
  const int s = blockIdx.z;
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *w = W.p[s] + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
  v2d b[LA_UNROLL];
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) b[u] = base + u * LA_BS < n ? w[base + u * LA_BS] : v2d{0.0, 0.0};
#pragma unroll 2
  for (int i = 0; i < nv; i++) {
    const v2d *vi = V.v[i][s] + off;
    const double cre = h[2 * i], cim = h[2 * i + 1];
#pragma unroll
    for (int u = 0; u < LA_UNROLL; u++)
      if (base + u * LA_BS < n) b[u] = tmhip_sub_cmul(b[u], cre, cim, vi[base + u * LA_BS]);
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++)
    if (base + u * LA_BS < n) { w[base + u * LA_BS] = b[u]; acc += b[u].x * b[u].x + b[u].y * b[u].y; }
  acc = tmhip_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < LA_BS / 64; q++) t += wsum[q];
    partials[(size_t)s * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// out = in / sqrt(*nrm2) (zero for a vector of norm zero: the breakdown is the host's to see)
__global__ __launch_bounds__(LA_BS, 8) void eig_scale_kernel(const Pair O, const Pair I, const double *__restrict__ nrm2, int ns, int n) {
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *o = O.p[blockIdx.z] + off;
  const v2d *in = I.p[blockIdx.z] + off;
  const double q = *nrm2, c = q > 0.0 ? 1.0 / sqrt(q) : 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) { const v2d a = in[i]; o[i] = v2d{c * a.x, c * a.y}; }
  }
}

// out = c1 x + c2 y [+ c3 z]; element-wise: out may be any input
__global__ __launch_bounds__(LA_BS, 8) void eig_cheb_kernel(const Pair O, const Pair X, const Pair Y, const Pair Z, double c1, double c2, double c3,
                                                            int ns, int n) {
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *o = O.p[blockIdx.z] + off;
  const v2d *x = X.p[blockIdx.z] + off, *y = Y.p[blockIdx.z] + off;
  const v2d *z = Z.p[blockIdx.z] ? Z.p[blockIdx.z] + off : nullptr;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) {
      const v2d a = x[i], b = y[i];
      v2d r = v2d{c1 * a.x + c2 * b.x, c1 * a.y + c2 * b.y};
      if (z) { const v2d c = z[i]; r = v2d{r.x + c3 * c.x, r.y + c3 * c.y}; }
      o[i] = r;
    }
  }
}

// V[:, 0:k] = V[:, 0:n] Y, Y real: a thread owns ONE complex element of a plane across all n vectors, reads its n values in ascending
// order while K accumulators stay in registers, and stores the k outputs after its last read -- in place without a work field.  Y lies
// in a device buffer as n rows of K doubles (zero beyond column k): the row of an input is uniform, so it arrives through scalar loads.
// K = 8 / 16 / 32 / 64 is chosen by the host as the smallest that holds k.
template <int K>
__global__ __launch_bounds__(LA_BS) void basis_rotate_kernel(const Basis V, int n, int k, const double *__restrict__ Y, int ns, int nsites) {
  const int e = blockIdx.x * LA_BS + threadIdx.x;
  if (e >= nsites) return;
  const int s = blockIdx.z;
  const size_t off = (size_t)blockIdx.y * ns + e;
  v2d acc[K];
#pragma unroll
  for (int c = 0; c < K; c++) acc[c] = v2d{0.0, 0.0};
#pragma unroll 2
  for (int i = 0; i < n; i++) {
    const v2d a = V.v[i][s][off];
    const double *y = Y + (size_t)i * K;
#pragma unroll
    for (int c = 0; c < K; c++) { acc[c].x = __builtin_fma(y[c], a.x, acc[c].x); acc[c].y = __builtin_fma(y[c], a.y, acc[c].y); }
  }
#pragma unroll
  for (int c = 0; c < K; c++)
    if (c < k) V.v[c][s][off] = acc[c];
}

// the default start vector: a fixed pseudo-random fill in (-1, 1), a hash of (segment, plane, site) -- the same on every call
__global__ __launch_bounds__(LA_BS) void eig_fill_kernel(const Pair O, int ns, int n) {
  const int e = blockIdx.x * LA_BS + threadIdx.x;
  if (e >= n) return;
  unsigned long long z = ((unsigned long long)(blockIdx.z * 64 + blockIdx.y) << 32) + (unsigned)e + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const double re = (double)(unsigned)(z & 0xffffffffu) * (2.0 / 4294967296.0) - 1.0 + 1.0 / 4294967296.0;
  const double im = (double)(unsigned)(z >> 32) * (2.0 / 4294967296.0) - 1.0 + 1.0 / 4294967296.0;
  O.p[blockIdx.z][(size_t)blockIdx.y * ns + e] = v2d{re, im};
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Vec { tmhip_field *f[2]; };   // f[1] == nullptr for a single flavour

// the shape of the vectors of a call
struct Shape { int kind, nseg, planes, n, ns; };

struct Work {
  int kind, nseg, count;        // what the vectors below are
  std::vector<Vec> v;           // basis (m + 1) and two work vectors; with "eig_fused" 0 the columns of a rotation behind them
  double *partials, *res_dev, *res_host, *y_dev;
  size_t partials_len;
  double lo, hi;                // tmhip_eig_set_interval (0, 0: automatic)
};

static Work *work_of(tmhip_ctx *ctx) {
  if (!ctx->eig) {
    Work *w = new Work();
    w->kind = -1; w->nseg = 0; w->count = 0;
    w->partials = w->res_dev = w->res_host = w->y_dev = nullptr;
    w->partials_len = 0; w->lo = w->hi = 0.0;
    w->v.reserve(2 * EIG_NV + 8);   // never reallocated: the driver keeps pointers into it while "eig_fused" 0 adds its columns
    ctx->eig = w;
  }
  return (Work *)ctx->eig;
}

static void free_vectors(tmhip_ctx *ctx, Work *w) {
  for (Vec &x : w->v) for (int s = 0; s < 2; s++) if (x.f[s]) tmhip_field_free(ctx, x.f[s]);
  w->v.clear();
  w->count = 0;
}

static void destroy(tmhip_ctx *ctx) {
  Work *w = (Work *)ctx->eig;
  if (!w) return;
  free_vectors(ctx, w);
  if (w->partials) (void)hipFree(w->partials);
  if (w->res_dev) (void)hipFree(w->res_dev);
  if (w->y_dev) (void)hipFree(w->y_dev);
  if (w->res_host) (void)hipHostFree(w->res_host);
  delete w;
  ctx->eig = nullptr;
}

#define EIG_RES (4 * EIG_NV + 8)   // doubles of the result block: the two passes of dots (2 EIG_NV each), then the norms
static int buffers(tmhip_ctx *ctx, Work *w) {
  if (w->partials) return 0;
  // a plane of at most Vh sites, 24 planes x 1 segment or 12 x 2, 2 EIG_NV values
  w->partials_len = (size_t)2 * EIG_NV * 24 * la_grid(ctx->Vh).x;
  TMHIP_CHECK(hipMalloc((void **)&w->partials, w->partials_len * sizeof(double)));
  TMHIP_CHECK(hipMalloc((void **)&w->res_dev, EIG_RES * sizeof(double)));
  TMHIP_CHECK(hipMalloc((void **)&w->y_dev, (size_t)TMHIP_EIG_MAX_BASIS * 64 * sizeof(double)));
  TMHIP_CHECK(hipHostMalloc((void **)&w->res_host, EIG_RES * sizeof(double)));
  return 0;
}

static int reserve(tmhip_ctx *ctx, Work *w, const Shape &sh, int count) {
  if (w->kind != sh.kind || w->nseg != sh.nseg) { free_vectors(ctx, w); w->kind = sh.kind; w->nseg = sh.nseg; }
  while ((int)w->v.size() < count) {
    Vec x = {{nullptr, nullptr}};
    w->v.push_back(x);
    Vec &y = w->v.back();
    for (int s = 0; s < sh.nseg; s++)
      if (tmhip_field_alloc(ctx, sh.kind, &y.f[s])) return 1;
  }
  w->count = (int)w->v.size();
  return 0;
}

static Pair pair_of(const Vec &x) { Pair p; p.p[0] = x.f[0]->d; p.p[1] = x.f[1] ? x.f[1]->d : nullptr; return p; }
static Basis basis_of(const Vec *v, int nv) {
  Basis b;
  memset(&b, 0, sizeof(b));
  for (int i = 0; i < nv; i++) { b.v[i][0] = v[i].f[0]->d; b.v[i][1] = v[i].f[1] ? v[i].f[1]->d : nullptr; }
  return b;
}
static dim3 grid_of(const Shape &sh) { return dim3(la_grid(sh.n).x, sh.planes, sh.nseg); }

// the EO fields a vector consists of, for the single entry points of linalg.hip ("eig_fused" 0): a FULL field is its two halves
static int eo_parts(const Vec &x, tmhip_field *out[2]) {
  if (x.f[0]->kind == TMHIP_FIELD_FULL) { out[0] = x.f[0]->half[0]; out[1] = x.f[0]->half[1]; return 2; }
  out[0] = x.f[0]; out[1] = x.f[1];
  return x.f[1] ? 2 : 1;
}

// ---- the pieces, enqueued on ctx->stream: results stay on the device
static int enqueue_dots(tmhip_ctx *ctx, Work *w, const Shape &sh, const Vec *v, int nv, const Vec &x, double *out_dev) {
  const dim3 g = grid_of(sh);
  hipLaunchKernelGGL(eig_dots_kernel, g, dim3(LA_BS), 0, ctx->stream, basis_of(v, nv), nv, pair_of(x), sh.ns, sh.n, w->partials);
  hipLaunchKernelGGL(eig_final_kernel, dim3(2 * nv), dim3(256), 0, ctx->stream, (const double *)w->partials, (int)(g.x * g.y), 2 * nv, sh.nseg, out_dev);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int enqueue_project(tmhip_ctx *ctx, Work *w, const Shape &sh, const Vec *v, int nv, const Vec &x, const double *h_dev, double *nrm_dev) {
  const dim3 g = grid_of(sh);
  hipLaunchKernelGGL(eig_project_kernel, g, dim3(LA_BS), 0, ctx->stream, basis_of(v, nv), nv, pair_of(x), h_dev, sh.ns, sh.n, w->partials);
  hipLaunchKernelGGL(eig_final_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double *)w->partials, (int)(g.x * g.y), 1, sh.nseg, nrm_dev);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int enqueue_rotate(tmhip_ctx *ctx, Work *w, const Shape &sh, const Vec *v, int n, int k, const double *Y /* n x k, row-major, host */) {
  const int K = k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64));
  std::vector<double> y((size_t)n * K, 0.0);
  for (int i = 0; i < n; i++) for (int c = 0; c < k; c++) y[(size_t)i * K + c] = Y[(size_t)i * k + c];
  // the stream has drained whenever the host arrives here with a new Y (every cycle ends with a synchronisation), so a plain copy is safe
  TMHIP_CHECK(hipMemcpyAsync(w->y_dev, y.data(), y.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  const dim3 g((sh.n + LA_BS - 1) / LA_BS, sh.planes, sh.nseg);
  const Basis b = basis_of(v, n);
  if (K == 8) hipLaunchKernelGGL(basis_rotate_kernel<8>, g, dim3(LA_BS), 0, ctx->stream, b, n, k, (const double *)w->y_dev, sh.ns, sh.n);
  else if (K == 16) hipLaunchKernelGGL(basis_rotate_kernel<16>, g, dim3(LA_BS), 0, ctx->stream, b, n, k, (const double *)w->y_dev, sh.ns, sh.n);
  else if (K == 32) hipLaunchKernelGGL(basis_rotate_kernel<32>, g, dim3(LA_BS), 0, ctx->stream, b, n, k, (const double *)w->y_dev, sh.ns, sh.n);
  else hipLaunchKernelGGL(basis_rotate_kernel<64>, g, dim3(LA_BS), 0, ctx->stream, b, n, k, (const double *)w->y_dev, sh.ns, sh.n);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int enqueue_comb(tmhip_ctx *ctx, const Shape &sh, const Vec &o, const Vec &x, const Vec &y, const Vec *z, double c1, double c2, double c3) {
  Pair zp; zp.p[0] = zp.p[1] = nullptr;
  if (z) zp = pair_of(*z);
  hipLaunchKernelGGL(eig_cheb_kernel, grid_of(sh), dim3(LA_BS), 0, ctx->stream, pair_of(o), pair_of(x), pair_of(y), zp, c1, c2, c3, sh.ns, sh.n);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}
static int copy_vec(tmhip_ctx *ctx, const Shape &sh, const Vec &dst, const Vec &src) {
  for (int s = 0; s < sh.nseg; s++)
    if (dst.f[s]->d != src.f[s]->d)
      TMHIP_CHECK(hipMemcpyAsync(dst.f[s]->d, src.f[s]->d, (size_t)sh.planes * sh.ns * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

// ---- the driver -----------------------------------------------------------------------------------------------------------------
struct Call {
  tmhip_ctx *ctx; Work *w; Shape sh;
  int op; bool nd;
  int m, fused, apps, max_apps;
};

static int apply(Call &c, const Vec &out, const Vec &in) {
  c.apps++;
  return c.nd ? tmhip_apply_nd_op(c.ctx, c.op, out.f[0], out.f[1], in.f[0], in.f[1]) : tmhip_apply_op(c.ctx, c.op, out.f[0], in.f[0]);
}

// x / |x| -> out (which may be x); *n2 = |x|^2
static int normalise(Call &c, const Vec &x, const Vec &out, double *n2) {
  tmhip_ctx *ctx = c.ctx; Work *w = c.w; const Shape &sh = c.sh;
  if (c.fused) {
    double *r = w->res_dev;
    if (enqueue_project(ctx, w, sh, &x, 0, x, r, r + 4 * EIG_NV + 1)) return 1;
    hipLaunchKernelGGL(eig_scale_kernel, grid_of(sh), dim3(LA_BS), 0, ctx->stream, pair_of(out), pair_of(x), (const double *)(r + 4 * EIG_NV + 1), sh.ns, sh.n);
    TMHIP_CHECK(hipGetLastError());
    TMHIP_CHECK(hipMemcpyAsync(w->res_host, r + 4 * EIG_NV + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n2 = w->res_host[0];
    return 0;
  }
  tmhip_field *xp[2], *op[2];
  const int np = eo_parts(x, xp);
  eo_parts(out, op);
  double t = 0.0;
  for (int s = 0; s < np; s++) { double q; if (tmhip_square_norm(ctx, xp[s], sh.n, 0, &q)) return 1; t = s == 0 ? q : t + q; }
  const double cs = t > 0.0 ? 1.0 / sqrt(t) : 0.0;
  for (int s = 0; s < np; s++) if (tmhip_mul_r(ctx, op[s], cs, xp[s], sh.n)) return 1;
  *n2 = t;
  return 0;
}

// x is made orthogonal to v[0 .. nv), nv >= 1, by classical Gram-Schmidt, twice; h[0 .. 2 nv) = the sums of the two passes'
// coefficients, *n1 and *n2 = |x|^2 after the first and after the second pass.  out (may be x itself, or null) = x / |x|.
// "eig_fused" 1: nine launches -- dots, project, dots, project, each followed by its one-block final pass, and the scaling --, everything
// on the device, ONE copy and synchronisation at the end.  "eig_fused" 0: tmhip_multi_scalar_prod in calls of up to TMHIP_CSG_MAX = 20
// fields (its kernel takes six per launch), one tmhip_assign_diff_mul per vector, tmhip_square_norm, tmhip_mul_r, per flavour.
static int orthonormalise(Call &c, const Vec *v, int nv, const Vec &x, const Vec *out, double *h, double *n1, double *n2) {
  tmhip_ctx *ctx = c.ctx; Work *w = c.w; const Shape &sh = c.sh;
  if (c.fused) {
    double *r = w->res_dev;
    if (enqueue_dots(ctx, w, sh, v, nv, x, r) || enqueue_project(ctx, w, sh, v, nv, x, r, r + 4 * EIG_NV)) return 1;
    if (enqueue_dots(ctx, w, sh, v, nv, x, r + 2 * EIG_NV) || enqueue_project(ctx, w, sh, v, nv, x, r + 2 * EIG_NV, r + 4 * EIG_NV + 1)) return 1;
    if (out) {
      hipLaunchKernelGGL(eig_scale_kernel, grid_of(sh), dim3(LA_BS), 0, ctx->stream, pair_of(*out), pair_of(x), (const double *)(r + 4 * EIG_NV + 1), sh.ns, sh.n);
      TMHIP_CHECK(hipGetLastError());
    }
    TMHIP_CHECK(hipMemcpyAsync(w->res_host, r, EIG_RES * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 2 * nv; i++) h[i] = w->res_host[i] + w->res_host[2 * EIG_NV + i];
    *n1 = w->res_host[4 * EIG_NV]; *n2 = w->res_host[4 * EIG_NV + 1];
    return 0;
  }
  // the same algorithm on the single entry points, with their host round trips
  tmhip_field *xp[2];
  const int np = eo_parts(x, xp);
  std::vector<double> hp(2 * nv), acc(2 * nv);
  std::vector<tmhip_field *> fs(nv);
  for (int i = 0; i < 2 * nv; i++) h[i] = 0.0;
  double nrm[2] = {0.0, 0.0};
  for (int pass = 0; pass < 2; pass++) {
    for (int i = 0; i < 2 * nv; i++) acc[i] = 0.0;
    for (int s = 0; s < np; s++) {
      for (int i = 0; i < nv; i++) { tmhip_field *p[2]; eo_parts(v[i], p); fs[i] = p[s]; }
      for (int first = 0; first < nv; first += TMHIP_CSG_MAX) {
        const int g = std::min(nv - first, TMHIP_CSG_MAX);
        if (tmhip_multi_scalar_prod(ctx, g, fs.data() + first, xp[s], sh.n, hp.data() + 2 * first)) return 1;
      }
      for (int i = 0; i < 2 * nv; i++) acc[i] = s == 0 ? hp[i] : acc[i] + hp[i];
    }
    for (int s = 0; s < np; s++)
      for (int i = 0; i < nv; i++) {
        tmhip_field *p[2]; eo_parts(v[i], p);
        const double cc[2] = {acc[2 * i], acc[2 * i + 1]};
        tmhip_field *r = xp[s];
        if (tmhip_multi_assign_diff_mul(ctx, 1, &r, p[s], cc, sh.n)) return 1;
      }
    for (int i = 0; i < 2 * nv; i++) h[i] += acc[i];
    double t = 0.0;
    for (int s = 0; s < np; s++) {
      double q;
      if (tmhip_square_norm(ctx, xp[s], sh.n, 0, &q)) return 1;
      t = s == 0 ? q : t + q;
    }
    nrm[pass] = t;
  }
  *n1 = nrm[0]; *n2 = nrm[1];
  if (out) {
    tmhip_field *op[2]; eo_parts(*out, op);
    const double cs = nrm[1] > 0.0 ? 1.0 / sqrt(nrm[1]) : 0.0;
    for (int s = 0; s < np; s++) if (tmhip_mul_r(ctx, op[s], cs, xp[s], sh.n)) return 1;
  }
  return 0;
}

// V[:, 0:k] = V[:, 0:n] Y.  "eig_fused" 0: one tmhip_lincomb per column and part into work vectors behind the basis, then copies back
static int rotate(Call &c, int n, int k, const double *Y) {
  Work *w = c.w;
  if (c.fused) return enqueue_rotate(c.ctx, w, c.sh, w->v.data(), n, k, Y);
  const int first_work = c.m + 3;
  if (reserve(c.ctx, w, c.sh, first_work + k)) return 1;
  std::vector<tmhip_field *> fs(n);
  std::vector<double> cc(2 * n);
  for (int col = 0; col < k; col++) {
    tmhip_field *dp[2]; const int np = eo_parts(w->v[first_work + col], dp);
    tmhip_field *tp[2]; eo_parts(w->v[first_work - 1], tp);   // the second work vector of the driver: free during a restart
    for (int s = 0; s < np; s++) {
      for (int i = 0; i < n; i++) { tmhip_field *p[2]; eo_parts(w->v[i], p); fs[i] = p[s]; cc[2 * i] = Y[(size_t)i * k + col]; cc[2 * i + 1] = 0.0; }
      for (int first = 0; first < n; first += TMHIP_CSG_MAX) {
        const int g = std::min(n - first, TMHIP_CSG_MAX);
        if (tmhip_lincomb(c.ctx, first == 0 ? dp[s] : tp[s], g, fs.data() + first, cc.data() + 2 * first, c.sh.n)) return 1;
        if (first && tmhip_add(c.ctx, dp[s], dp[s], tp[s], c.sh.n)) return 1;
      }
    }
  }
  for (int col = 0; col < k; col++) if (copy_vec(c.ctx, c.sh, w->v[col], w->v[first_work + col])) return 1;
  TMHIP_CHECK(hipStreamSynchronize(c.ctx->stream));
  while ((int)w->v.size() > first_work) {   // the baseline's extra columns do not stay
    for (int s = 0; s < 2; s++) if (w->v.back().f[s]) tmhip_field_free(c.ctx, w->v.back().f[s]);
    w->v.pop_back();
  }
  w->count = first_work;
  return 0;
}

// out = B in, B = A (deg 0) or T_deg((hi + lo - 2 A) / (hi - lo)); `out` is one of the three buffers buf[0..2] and may not be `in`
static int apply_filtered(Call &c, int deg, double lo, double hi, const Vec &out, const Vec &in, const Vec &w0, const Vec &w1) {
  if (deg <= 0) return apply(c, out, in);
  const double a = -2.0 / (hi - lo), cc = (hi + lo) / (hi - lo);
  const Vec *buf[3] = {&out, &w0, &w1};   // t_k lives in buf[(deg - k) % 3]: t_deg in `out`
  const Vec *tprev = nullptr, *tcur = &in;
  for (int k = 1; k <= deg; k++) {
    const Vec *tn = buf[(deg - k) % 3];
    if (apply(c, *tn, *tcur)) return 1;
    if (k == 1) { if (enqueue_comb(c.ctx, c.sh, *tn, *tn, *tcur, nullptr, a, cc, 0.0)) return 1; }
    else if (enqueue_comb(c.ctx, c.sh, *tn, *tn, *tcur, tprev, 2.0 * a, 2.0 * cc, -1.0)) return 1;
    tprev = tcur; tcur = tn;
  }
  return 0;
}

struct Result { std::vector<double> evals, resid; int converged; };

// theta_i = <v_i, A v_i> and |A v_i - theta_i v_i| for the unit vectors v[0 .. cnt): one application each, the residual through the
// project kernel with the Rayleigh quotient as its coefficient
static int true_residuals(Call &c, int cnt, double *theta, double *res) {
  Work *w = c.w;
  const int m1 = c.m + 1;   // the first work vector
  for (int i = 0; i < cnt; i++) {
    double h[2], n1;
    if (apply(c, w->v[m1], w->v[i])) return 1;
    if (c.fused) {
      double *r = w->res_dev;
      if (enqueue_dots(c.ctx, w, c.sh, &w->v[i], 1, w->v[m1], r) || enqueue_project(c.ctx, w, c.sh, &w->v[i], 1, w->v[m1], r, r + 4 * EIG_NV)) return 1;
      TMHIP_CHECK(hipMemcpyAsync(w->res_host, r, EIG_RES * sizeof(double), hipMemcpyDeviceToHost, c.ctx->stream));
      TMHIP_CHECK(hipStreamSynchronize(c.ctx->stream));
      h[0] = w->res_host[0]; n1 = w->res_host[4 * EIG_NV];
    } else {
      // one pass only: a second one would fold the residual's own component along v_i into theta
      tmhip_field *xp[2], *vp[2];
      const int np = eo_parts(w->v[m1], xp);
      eo_parts(w->v[i], vp);
      double acc[2] = {0.0, 0.0};
      for (int s = 0; s < np; s++) { double q[2]; if (tmhip_multi_scalar_prod(c.ctx, 1, &vp[s], xp[s], c.sh.n, q)) return 1; acc[0] = s ? acc[0] + q[0] : q[0]; acc[1] = s ? acc[1] + q[1] : q[1]; }
      n1 = 0.0;
      for (int s = 0; s < np; s++) {
        double q;
        if (tmhip_multi_assign_diff_mul(c.ctx, 1, &xp[s], vp[s], acc, c.sh.n) || tmhip_square_norm(c.ctx, xp[s], c.sh.n, 0, &q)) return 1;
        n1 = s ? n1 + q : q;
      }
      h[0] = acc[0];
    }
    theta[i] = h[0];
    res[i] = sqrt(n1);
  }
  return 0;
}

// One thick-restart Lanczos run on B = filter(A) from the unit start vector in v[0].  `largest`: the wanted end of B.  Ends when the
// nev wanted pairs meet `prec` on the true residual with A, when the operator-application cap leaves no room for another step, after
// `max_restarts` restarts, or -- `one_cycle` -- after the first cycle (whose Ritz values of B then come back in ritz / ritz_res, ascending).
// On exit v[0 .. got) are the wanted Ritz vectors, best first.
static int lanczos(Call &c, int m, int nev, bool largest, int deg, double lo, double hi, double prec, int max_restarts, bool one_cycle,
                   std::vector<double> *ritz, std::vector<double> *ritz_res, int *keep_rule, int *got, double *theta, double *res, int *converged) {
  Work *w = c.w;
  Vec *v = w->v.data();
  const Vec &w0 = v[m + 1], &w1 = v[m + 2];
  const int step_cost = deg > 0 ? deg : 1;
  std::vector<double> T((size_t)m * m, 0.0), S((size_t)m * m), th(m), h(2 * EIG_NV), Y;
  int k = 0;        // vectors kept from the last restart; v[k] is the residual vector
  bool fresh = false;   // theta / res hold the computed residuals of v[0 .. *got) as they stand
  double anorm = 0.0;
  *converged = 0; *got = 0;
  for (int restart = 0;; restart++) {
    int len = k;
    bool broke = false, capped = false;
    double beta = 0.0;
    for (int j = k; j < m; j++) {
      if (c.apps + step_cost + nev > c.max_apps) { capped = true; break; }
      if (apply_filtered(c, deg, lo, hi, v[j + 1], v[j], w0, w1)) return 1;
      double n1, n2;
      if (orthonormalise(c, v, j + 1, v[j + 1], &v[j + 1], h.data(), &n1, &n2)) return 1;
      const double alpha = h[2 * j];
      T[(size_t)j * m + j] = alpha;
      beta = sqrt(n2);
      // |B v_j|^2 = |h|^2 + n2: the norm before the orthogonalisation, and a running estimate of |B|
      double before = n2;
      for (int i = 0; i <= j; i++) before += h[2 * i] * h[2 * i] + h[2 * i + 1] * h[2 * i + 1];
      before = sqrt(before);
      anorm = std::max(anorm, before);
      len = j + 1;
      if (!(beta > 1e-14 * anorm)) { broke = true; beta = 0.0; break; }   // an invariant subspace: the cycle ends at this length
      if (j + 1 < m) T[(size_t)j * m + j + 1] = T[(size_t)(j + 1) * m + j] = beta;
    }
    if (len == k && capped) {
      // no room for another step: what the last restart kept (or the start vector alone) is the answer
      *got = std::min(nev, std::max(k, 1));
      if (one_cycle) { if (ritz) { ritz->clear(); ritz_res->clear(); } return 0; }   // no cycle, no Ritz values: the caller runs unfiltered
      if (fresh) return 0;   // the restart before this one has just computed them: the cap includes the residuals' applications
      if (true_residuals(c, *got, theta, res)) return 1;
      *converged = 0;
      for (int q = 0; q < *got; q++) if (res[q] <= prec) (*converged)++;
      return 0;
    }
    // the projected matrix of this cycle: the leading len x len block of T
    for (int i = 0; i < len; i++) for (int j = 0; j < len; j++) S[(size_t)i * len + j] = T[(size_t)i * m + j];
    if (tmhip_eig_small_jacobi(len, S.data(), th.data())) TMHIP_FAIL("eigenvalues: the projected eigenproblem did not converge");
    if (ritz) {
      ritz->assign(th.begin(), th.begin() + len);
      ritz_res->resize(len);
      for (int i = 0; i < len; i++) (*ritz_res)[i] = fabs(beta * S[(size_t)(len - 1) * len + i]);
    }
    // how many Ritz vectors the restart keeps: nev + (m - nev) / 2, capped at m - 2 and by what the cycle has
    int keep = nev + (m - nev) / 2;
    if (keep > m - 2) keep = m - 2;
    if (keep > len - 1) keep = len - 1;
    if (keep < 1) keep = 1;
    if (keep_rule) *keep_rule = keep;
    const bool last = broke || capped || one_cycle || restart >= max_restarts;
    if (last && keep < std::min(nev, len)) keep = std::min(nev, len);
    // wanted first: column `col(i)` of S is the i-th wanted Ritz vector
    auto col = [&](int i) { return largest ? len - 1 - i : i; };
    Y.assign((size_t)len * keep, 0.0);
    for (int i = 0; i < len; i++) for (int q = 0; q < keep; q++) Y[(size_t)i * keep + q] = S[(size_t)i * len + col(q)];
    // Lanczos estimates of the wanted pairs (of B): |beta s_{len-1, i}|
    bool est_ok = true;
    for (int q = 0; q < std::min(nev, keep); q++) est_ok = est_ok && fabs(beta * S[(size_t)(len - 1) * len + col(q)]) <= prec;
    if (rotate(c, len, keep, Y.data())) return 1;
    *got = std::min(nev, keep);
    const bool check = last || deg > 0 || est_ok;
    if (check && !one_cycle) {
      if (true_residuals(c, *got, theta, res)) return 1;
      int conv = 0;
      for (int q = 0; q < *got; q++) if (res[q] <= prec) conv++;
      *converged = conv;
      fresh = true;
      if (conv == nev || last) return 0;
    } else {
      fresh = false;
      if (last) return 0;
    }
    // restart: v[keep] = the residual vector, T = diag(theta) with the arrow beta s_{len-1, i}
    if (copy_vec(c.ctx, c.sh, v[keep], v[len])) return 1;
    std::fill(T.begin(), T.end(), 0.0);
    for (int q = 0; q < keep; q++) {
      T[(size_t)q * m + q] = th[col(q)];
      T[(size_t)q * m + keep] = T[(size_t)keep * m + q] = beta * S[(size_t)(len - 1) * len + col(q)];
    }
    k = keep;
  }
}

static int run(tmhip_ctx *ctx, const char *who, bool nd, int op, const Shape &sh, int nev, int which, double prec, int max_apps,
               tmhip_field *const *evec_up, tmhip_field *const *evec_dn, double *evals, double *resid, int *converged, int *apps) {
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: T-split ranks (and their loopback rehearsal) are not built: the sums are rank-local", who);
  if (!evals || !resid || !converged || !apps) TMHIP_FAIL("%s: null argument", who);
  const int m = ctx->opt_eig_basis;
  if (m > TMHIP_EIG_MAX_BASIS) TMHIP_FAIL("%s: eig_basis = %d exceeds TMHIP_EIG_MAX_BASIS = %d", who, m, TMHIP_EIG_MAX_BASIS);
  if (nev < 1 || nev + 2 > m) TMHIP_FAIL("%s: nev = %d needs nev >= 1 and nev + 2 <= eig_basis = %d", who, nev, m);
  if (which != 0 && which != 1) TMHIP_FAIL("%s: which = %d is neither 0 (lowest) nor 1 (highest)", who, which);
  if (!(prec > 0.0)) TMHIP_FAIL("%s: prec must be positive", who);
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  const int deg = which == 0 ? ctx->opt_eig_cheb : 0;
  if (max_apps < nev + 1) TMHIP_FAIL("%s: max_apps = %d is too small for nev = %d (at least nev + 1)", who, max_apps, nev);
  for (int i = 0; i < nev; i++) {
    if (evec_up) {
      tmhip_field *f = evec_up[i];
      if (!f || f->prec || f->kind != sh.kind || f->ns != sh.ns || f->view) TMHIP_FAIL("%s: evec[%d] is not an fp64 field of the operator's kind", who, i);
    }
    if (evec_dn) {
      tmhip_field *f = evec_dn[i];
      if (!evec_up || !f || f->prec || f->kind != sh.kind || f->ns != sh.ns || f->d == evec_up[i]->d) TMHIP_FAIL("%s: evec_dn[%d] is not a field of its own of the operator's kind", who, i);
    }
  }
  if (nd && evec_up && !evec_dn) TMHIP_FAIL("%s: the doublet's eigenvectors need both evec_up and evec_dn", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  if (buffers(ctx, w) || reserve(ctx, w, sh, m + 3)) return 1;
  Call c;
  c.ctx = ctx; c.w = w; c.sh = sh; c.op = op; c.nd = nd; c.m = m; c.fused = ctx->opt_eig_fused; c.apps = 0; c.max_apps = max_apps;
  Vec *v = w->v.data();
  // the start vector: evec[0] when it is given with a non-zero norm, else the fixed pseudo-random fill
  bool have_start = false;
  if (evec_up) {
    Vec s0 = {{evec_up[0], nd ? evec_dn[0] : nullptr}};
    if (copy_vec(ctx, sh, v[m + 1], s0)) return 1;
    double n2;
    if (normalise(c, v[m + 1], v[0], &n2)) return 1;
    have_start = n2 > 0.0 && std::isfinite(n2);
  }
  if (!have_start) {
    hipLaunchKernelGGL(eig_fill_kernel, dim3((sh.n + LA_BS - 1) / LA_BS, sh.planes, sh.nseg), dim3(LA_BS), 0, ctx->stream, pair_of(v[m + 1]), sh.ns, sh.n);
    TMHIP_CHECK(hipGetLastError());
    double n2;
    if (normalise(c, v[m + 1], v[0], &n2)) return 1;
  }
  std::vector<double> theta(nev, 0.0), res(nev, 0.0);
  int got = 0, conv = 0;
  double lo = w->lo, hi = w->hi;
  if (deg > 0 && !(hi > lo)) {
    // the interval from one unfiltered cycle: hi = 1.1 (largest Ritz value + its residual bound); lo = the largest Ritz value the restart
    // rule would keep -- by interlacing the i-th Ritz value from below is >= the i-th eigenvalue, so every wanted eigenvalue is below lo
    std::vector<double> ritz, rres;
    int keep = 0;
    if (lanczos(c, m, nev, false, 0, 0.0, 0.0, prec, 0, true, &ritz, &rres, &keep, &got, theta.data(), res.data(), &conv)) return 1;
    const int len = (int)ritz.size();
    if (len >= nev + 2) {
      hi = 1.1 * (ritz[len - 1] + rres[len - 1]);
      lo = ritz[std::min(keep, len) - 1];
    }
    // a cycle the cap cut short (or did not allow at all), or an invariant subspace smaller than the basis: nothing to filter, run plain
    if (!(hi > lo) || len < nev + 2) { lo = hi = 0.0; }
    else {
      // the filtered run starts from the sum of the nev lowest Ritz vectors, v[0 .. nev) after the cycle's rotation
      std::vector<double> y(nev, 1.0 / sqrt((double)nev));
      if (rotate(c, nev, 1, y.data())) return 1;
    }
  }
  const bool filtered = deg > 0 && hi > lo;
  const int max_restarts = ctx->opt_eig_restarts > 0 ? ctx->opt_eig_restarts - 1 : 1 << 30;   // "eig_restarts" cycles: the last one is number eig_restarts - 1
  if (lanczos(c, m, nev, filtered ? true : which == 1, filtered ? deg : 0, lo, hi, prec, max_restarts, false, nullptr, nullptr, nullptr, &got, theta.data(),
              res.data(), &conv)) return 1;
  // ascending for the lowest end, descending for the highest; the vectors follow
  std::vector<int> order(got);
  for (int i = 0; i < got; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return which == 0 ? theta[a] < theta[b] : theta[a] > theta[b]; });
  for (int i = 0; i < nev; i++) {
    if (i < got) { evals[i] = theta[order[i]]; resid[i] = res[order[i]]; }
    else { evals[i] = theta[order[got - 1]]; resid[i] = HUGE_VAL; }   // fewer vectors than nev (cap or invariant subspace): never counted as converged
  }
  if (evec_up)
    for (int i = 0; i < got; i++) {
      Vec d = {{evec_up[i], nd ? evec_dn[i] : nullptr}};
      if (copy_vec(ctx, sh, d, v[order[i]])) return 1;
    }
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *converged = conv;
  *apps = c.apps;
  return 0;
}

static int check_vecs(const char *who, int n, tmhip_field *const *a, tmhip_field *const *b, const tmhip_field *w0, Shape *sh, tmhip_ctx *ctx, int N) {
  if (!w0 || w0->prec || w0->view) TMHIP_FAIL("%s: needs fp64 fields of their own", who);
  sh->kind = w0->kind; sh->nseg = b ? 2 : 1; sh->ns = w0->ns;
  if (w0->kind == TMHIP_FIELD_FULL) {
    if (b) TMHIP_FAIL("%s: a doublet is a pair of one-parity (EO) fields", who);
    if (N != ctx->V) TMHIP_FAIL("%s: N = %d, FULL fields take N = VOLUME = %d", who, N, ctx->V);
    sh->planes = 24; sh->n = ctx->Vh;
  } else {
    if (N < 1 || N > ctx->Vh) TMHIP_FAIL("%s: N = %d is outside [1, VOLUME/2 = %d]", who, N, ctx->Vh);
    sh->planes = 12; sh->n = N;
  }
  for (int i = 0; i < n; i++) {
    if (!a || !a[i] || a[i]->prec || a[i]->kind != sh->kind || a[i]->ns != sh->ns) TMHIP_FAIL("%s: v[%d] is not an fp64 field of the kind of w", who, i);
    if (b && (!b[i] || b[i]->prec || b[i]->kind != sh->kind || b[i]->ns != sh->ns)) TMHIP_FAIL("%s: v_dn[%d] is not an fp64 field of the kind of w", who, i);
  }
  return 0;
}

static std::vector<Vec> vecs_of(int n, tmhip_field *const *a, tmhip_field *const *b) {
  std::vector<Vec> v(n > 0 ? n : 1);
  for (int i = 0; i < n; i++) { v[i].f[0] = a[i]; v[i].f[1] = b ? b[i] : nullptr; }
  return v;
}

}  // namespace eighip

void tmhip_eig_destroy(tmhip_ctx *ctx) { eighip::destroy(ctx); }

extern "C" {

int tmhip_eig_small(int n, double *A, double *w) {
  if (n < 1 || n > TMHIP_EIG_MAX_BASIS) TMHIP_FAIL("eig_small: n = %d is outside [1, %d]", n, TMHIP_EIG_MAX_BASIS);
  if (tmhip_eig_small_jacobi(n, A, w)) TMHIP_FAIL("eig_small: the Jacobi sweeps did not converge");
  return 0;
}

int tmhip_eig_set_interval(tmhip_ctx *ctx, double lo, double hi) {
  if (!(lo == 0.0 && hi == 0.0) && !(hi > lo && lo > 0.0)) TMHIP_FAIL("eig_set_interval: needs 0 < lo < hi, or 0, 0 for the automatic interval");
  eighip::Work *w = eighip::work_of(ctx);
  w->lo = lo; w->hi = hi;
  return 0;
}

int tmhip_eig_dots(tmhip_ctx *ctx, int nv, tmhip_field *const *v_up, tmhip_field *const *v_dn, tmhip_field *w_up, tmhip_field *w_dn, int N, double *out) {
  using namespace eighip;
  if (nv < 1 || nv > EIG_NV) TMHIP_FAIL("eig_dots: %d vectors, must be in [1, %d]", nv, EIG_NV);
  if (!out || (!v_dn) != (!w_dn)) TMHIP_FAIL("eig_dots: null argument");
  Shape sh;
  if (check_vecs("eig_dots", nv, v_up, v_dn, w_up, &sh, ctx, N)) return 1;
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("eig_dots: rank-local; T-split ranks are not built");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  if (buffers(ctx, w)) return 1;
  std::vector<Vec> v = vecs_of(nv, v_up, v_dn);
  Vec x = {{w_up, w_dn}};
  if (enqueue_dots(ctx, w, sh, v.data(), nv, x, w->res_dev)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(w->res_host, w->res_dev, 2 * nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  memcpy(out, w->res_host, 2 * nv * sizeof(double));
  return 0;
}

int tmhip_eig_project(tmhip_ctx *ctx, int nv, tmhip_field *const *v_up, tmhip_field *const *v_dn, tmhip_field *w_up, tmhip_field *w_dn, const double *h, int N,
                      double *sqnorm) {
  using namespace eighip;
  if (nv < 1 || nv > EIG_NV) TMHIP_FAIL("eig_project: %d vectors, must be in [1, %d]", nv, EIG_NV);
  if (!h || !sqnorm || (!v_dn) != (!w_dn)) TMHIP_FAIL("eig_project: null argument");
  Shape sh;
  if (check_vecs("eig_project", nv, v_up, v_dn, w_up, &sh, ctx, N)) return 1;
  for (int i = 0; i < nv; i++)
    if (v_up[i]->d == w_up->d || (v_dn && (v_dn[i]->d == w_dn->d || v_dn[i]->d == w_up->d || v_up[i]->d == w_dn->d)))
      TMHIP_FAIL("eig_project: w is v[%d] (other blocks of the launch read it)", i);
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("eig_project: rank-local; T-split ranks are not built");
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  if (buffers(ctx, w)) return 1;
  std::vector<Vec> v = vecs_of(nv, v_up, v_dn);
  Vec x = {{w_up, w_dn}};
  TMHIP_CHECK(hipMemcpyAsync(w->res_dev, h, 2 * nv * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (enqueue_project(ctx, w, sh, v.data(), nv, x, w->res_dev, w->res_dev + 4 * EIG_NV)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(w->res_host, w->res_dev + 4 * EIG_NV, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *sqnorm = w->res_host[0];
  return 0;
}

int tmhip_basis_rotate(tmhip_ctx *ctx, int n, int k, tmhip_field *const *v_up, tmhip_field *const *v_dn, const double *Y, int N) {
  using namespace eighip;
  if (n < 1 || n > TMHIP_EIG_MAX_BASIS || k < 1 || k > n) TMHIP_FAIL("basis_rotate: n = %d, k = %d, needs 1 <= k <= n <= %d", n, k, TMHIP_EIG_MAX_BASIS);
  if (!Y || !v_up) TMHIP_FAIL("basis_rotate: null argument");
  Shape sh;
  if (check_vecs("basis_rotate", n, v_up, v_dn, v_up[0], &sh, ctx, N)) return 1;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      if (i < j && v_up[i]->d == v_up[j]->d) TMHIP_FAIL("basis_rotate: v[%d] is v[%d]", i, j);
      if (v_dn && ((i < j && v_dn[i]->d == v_dn[j]->d) || v_dn[i]->d == v_up[j]->d)) TMHIP_FAIL("basis_rotate: the two flavours share a field");
    }
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = work_of(ctx);
  if (buffers(ctx, w)) return 1;
  std::vector<Vec> v = vecs_of(n, v_up, v_dn);
  if (enqueue_rotate(ctx, w, sh, v.data(), n, k, Y)) return 1;
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tmhip_eigenvalues(tmhip_ctx *ctx, int op, int N, int nev, int which, double prec, int max_apps, tmhip_field *const *evec, double *evals, double *resid,
                      int *converged, int *apps) {
  const tmhip_op_row *r = tmhip_op_row_of(op);
  if (tmhip_op_check(ctx, "eigenvalues", TMHIP_S_EIG, op, r ? r->kind : TMHIP_FIELD_EO)) return 1;
  eighip::Shape sh;
  sh.kind = r->kind; sh.nseg = 1; sh.ns = ctx->ns;
  if (r->kind == TMHIP_FIELD_FULL) {
    if (N != ctx->V) TMHIP_FAIL("eigenvalues: N = %d, %s takes N = VOLUME = %d", N, r->name, ctx->V);
    sh.planes = 24;
  } else {
    if (N != ctx->Vh) TMHIP_FAIL("eigenvalues: N = %d, %s takes N = VOLUME/2 = %d", N, r->name, ctx->Vh);
    sh.planes = 12;
  }
  sh.n = ctx->Vh;
  return eighip::run(ctx, "eigenvalues", false, op, sh, nev, which, prec, max_apps, evec, nullptr, evals, resid, converged, apps);
}

int tmhip_eigenvalues_nd(tmhip_ctx *ctx, int op, int nev, int which, double prec, int max_apps, tmhip_field *const *evec_up, tmhip_field *const *evec_dn,
                         double *evals, double *resid, int *converged, int *apps) {
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("eigenvalues_nd: the doublet is not built for T-split lattices");
  if (tmhip_nd_op_check(ctx, "eigenvalues_nd", op)) return 1;
  eighip::Shape sh;
  sh.kind = TMHIP_FIELD_EO; sh.nseg = 2; sh.ns = ctx->ns; sh.planes = 12; sh.n = ctx->Vh;
  return eighip::run(ctx, "eigenvalues_nd", true, op, sh, nev, which, prec, max_apps, evec_up, evec_dn, evals, resid, converged, apps);
}

}  // extern "C"
