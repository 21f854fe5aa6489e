// bicgstab_complex (solver/bicgstab_complex.c:49-116) kept entirely in HBM.
//
// The reference's loop needs five complex scalars per iteration on the host (denom, omega, its norm, rho1 and err) and walks its
// six work fields about 26 times beside the two operator applications.  Here the scalars live in a small device state block (as
// CgState of cg.hip), the vector work between the two stencils is five kernels with 18 field passes, every kernel reads its
// coefficients from the state and skips its work once `done` is set, and the host only enqueues (tmhip_poll_loop):
//   v = A p
//   K1  <hatr, v>                                  alpha = rho0 / <hatr, v>                      :91-92
//   K2  s = r - alpha v                                                                          :93-94
//   t = A s
//   K3  <t, s> and <t, t> in one pass over t       omega = <t, s> / <t, t>                       :96-97
//   K4  P += alpha p + omega s ; r = s - omega t ; <hatr, r> and <r, r> of the r just computed   :98-101, :80
//       rho1, err, the breakdown test of :102, beta = alpha rho1 / (omega rho0), rho0 = rho1, the stopping test of :86
//   K5  p = beta (p - omega v) + r                                                               :110-111
// The element operations are those of the singles (tmhip_internal.h) and the sums keep the singles' layout -- per-thread order,
// wave butterfly, the waves of a block, one block sum per (value, plane, block), the fixed-order final pass of reduce_final_kernel
// (linalg.hip) --, so with the same scalars a fused kernel leaves the bits of the calls it replaces and a sum the bits of
// tmhip_scalar_prod / tmhip_square_norm.  FULL fields (D_psi) are twenty-four planes; their sums are taken half by half and added,
// even first, which is what the singles give on the two halves.
#include "tmhip_internal.h"

namespace bicghip {

struct BicgState {
  double rho0[2], alpha[2], omega[2], nomega[2], beta[2];   // nomega = -omega: the c1 of assign_mul_bra_add_mul_ket_add (:110)
  double err, squarenorm, eps_sq;
  int rel_prec, done, iters, it, max_iter, pad;
};

struct Work {
  tmhip_field *f[2][6];   // [field kind][hatr, r, v, p, s, t]
  BicgState *st;          // [0] the solver's state, [1] the state of the entry points with host scalars
  double *partials;       // [3 values][24 planes][blocks]
  double *sums;           // [3], device
  double *sums_host;      // pinned
  double *hist; int hist_len;
};

// (a + i b) / (c + i d) without forming c^2 + d^2 (Smith): one formula for the device state and the host loop of "bicg_fused" 0
__host__ __device__ inline void cdiv(const double n[2], const double d[2], double q[2]) {
  if (fabs(d[0]) >= fabs(d[1])) {
    const double r = d[1] / d[0], den = d[0] + d[1] * r;
    q[0] = (n[0] + n[1] * r) / den; q[1] = (n[1] - n[0] * r) / den;
  } else {
    const double r = d[0] / d[1], den = d[0] * r + d[1];
    q[0] = (n[0] * r + n[1]) / den; q[1] = (n[1] * r - n[0]) / den;
  }
}
__host__ __device__ inline void cmulh(const double a[2], const double b[2], double p[2]) {
  const double re = a[0] * b[0] - a[1] * b[1], im = a[0] * b[1] + a[1] * b[0];
  p[0] = re; p[1] = im;
}
__host__ __device__ inline bool converged(double err, double eps_sq, double squarenorm, int rel_prec) {
  return ((err <= eps_sq) && (rel_prec == 0)) || ((err <= eps_sq * squarenorm) && (rel_prec == 1));
}
// the scalar lines of an iteration, shared by the device state and the host loop.  after_K1: :92; after_K3: :96-97; after_K4: :102-112
// and the test of :86 for the iteration that follows (it = the number of completed iterations); returns true when the solve ends
__host__ __device__ inline void after_K1(BicgState &s, const double denom[2]) { cdiv(s.rho0, denom, s.alpha); }
__host__ __device__ inline void after_K3(BicgState &s, const double ts[2], double tt) {
  s.omega[0] = ts[0] / tt; s.omega[1] = ts[1] / tt;
  s.nomega[0] = -s.omega[0]; s.nomega[1] = -s.omega[1];
}
__host__ __device__ inline bool after_K4(BicgState &s, const double rho1[2], double err) {
  s.err = err;
  s.it += 1;
  if (fabs(rho1[0]) < 1.e-25 && fabs(rho1[1]) < 1.e-25) { s.done = 1; s.iters = -1; return true; }
  double nom[2], denom[2];
  cmulh(s.alpha, rho1, nom);
  cmulh(s.omega, s.rho0, denom);
  cdiv(nom, denom, s.beta);
  s.rho0[0] = rho1[0]; s.rho0[1] = rho1[1];
  if (s.it < s.max_iter && converged(err, s.eps_sq, s.squarenorm, s.rel_prec)) { s.done = 1; s.iters = s.it; return true; }
  return false;
}

// block sums of NV values into partials[(k * gridDim.y + plane) * gridDim.x + block]: per value the lines of block_reduce_store (linalg.hip)
template <int NV>
__device__ __forceinline__ void block_sums_store(const double (&v)[NV], double *partials) {
  __shared__ double wsum[NV][LA_BS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const double a = tmhip_wave_sum(v[k]);
    if (lane == 0) wsum[k][w] = a;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_BS / 64; k++) s += wsum[threadIdx.x][k];
    partials[((size_t)threadIdx.x * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
  }
}

// K1 (NORM false): values 0, 1 = Re, Im <A, B>.  K3 (NORM true): the same and value 2 = <A, A>, A read once.
template <bool NORM>
__global__ __launch_bounds__(LA_BS, 8) void dot_kernel(const v2d *__restrict__ A, const v2d *__restrict__ B, int ns, int n, double *partials,
                                                       const BicgState *__restrict__ st) {
  if (st->done) return;
  const size_t off = (size_t)blockIdx.y * ns;
  const v2d *a = A + off, *b = B + off;
  double acc[NORM ? 3 : 2];
#pragma unroll
  for (int k = 0; k < (NORM ? 3 : 2); k++) acc[k] = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) {
      const v2d x = a[i], y = b[i];
      tmhip_cdot_add(acc[0], acc[1], x, y);
      if (NORM) acc[2] += tmhip_norm2(x);
    }
  }
  block_sums_store(acc, partials);
}

// K2: s = r - alpha v   (assign, assign_diff_mul)
__global__ __launch_bounds__(LA_BS, 8) void sub_kernel(v2d *__restrict__ S, const v2d *__restrict__ R, const v2d *__restrict__ V, int ns, int n,
                                                       const BicgState *__restrict__ st) {
  if (st->done) return;
  const double are = st->alpha[0], aim = st->alpha[1];
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *s = S + off;
  const v2d *r = R + off, *v = V + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) s[i] = tmhip_sub_cmul(r[i], are, aim, v[i]);
  }
}

// K4: P += alpha p + omega s ; r = s - omega t ; values 0, 1 = <hatr, r>, 2 = <r, r> of the r just stored
__global__ __launch_bounds__(LA_BS, 8) void update_kernel(v2d *__restrict__ X, v2d *__restrict__ R, const v2d *__restrict__ Pd, const v2d *__restrict__ S,
                                                          const v2d *__restrict__ Tt, const v2d *__restrict__ H, int ns, int n, double *partials,
                                                          const BicgState *__restrict__ st) {
  if (st->done) return;
  const double are = st->alpha[0], aim = st->alpha[1], ore = st->omega[0], oim = st->omega[1];
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *x = X + off, *r = R + off;
  const v2d *p = Pd + off, *s = S + off, *t = Tt + off, *h = H + off;
  double acc[3] = {0.0, 0.0, 0.0};
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) {
      const v2d sv = s[i];
      x[i] = tmhip_add_mul_add_mul(x[i], are, aim, p[i], ore, oim, sv);
      const v2d rv = tmhip_sub_cmul(sv, ore, oim, t[i]);
      r[i] = rv;
      tmhip_cdot_add(acc[0], acc[1], h[i], rv);
      acc[2] += tmhip_norm2(rv);
    }
  }
  block_sums_store(acc, partials);
}

// K5: p = beta (p - omega v) + r   (assign_mul_bra_add_mul_ket_add with c1 = -omega, c2 = beta)
__global__ __launch_bounds__(LA_BS, 8) void dir_kernel(v2d *__restrict__ Pd, const v2d *__restrict__ V, const v2d *__restrict__ R, int ns, int n,
                                                       const BicgState *__restrict__ st) {
  if (st->done) return;
  const double c1re = st->nomega[0], c1im = st->nomega[1], c2re = st->beta[0], c2im = st->beta[1];
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *p = Pd + off;
  const v2d *v = V + off, *r = R + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < n) p[i] = tmhip_mul_bra_add_mul_ket_add(p[i], c1re, c1im, v[i], c2re, c2im, r[i]);
  }
}

// The final pass and the scalar step of a reduction in one launch of one block: its four groups of 256 threads each add up one
// (value, half) -- `per` block sums, in the order of reduce_final_kernel (linalg.hip) --, the halves of a value are added, even
// first, and thread 0 moves the state on.  WHICH 0: the sums only (the entry points with host scalars), 1 / 3 / 4: after K1 / K3 / K4.
template <int WHICH>
__global__ __launch_bounds__(1024) void sum_scalar_kernel(const double *__restrict__ partials, int per, int halves, BicgState *st, double *sums,
                                                          double *hist, int hist_len) {
  constexpr int NV = WHICH == 1 ? 2 : 3;
  __shared__ double sm[4][256];
  __shared__ double res[2 * NV];
  if (st->done) return;   // block-uniform: written by an earlier launch only
  const int g = threadIdx.x >> 8, l = threadIdx.x & 255;
  const int nsum = NV * halves;
  for (int first = 0; first < nsum; first += 4) {
    const int q = first + g;   // sum q = value q / halves, half q % halves: the partials of a value's halves lie one after the other
    double acc = 0.0;
    if (q < nsum) {
      const double *p = partials + (size_t)q * per;
      for (int i = l; i < per; i += 256) acc += p[i];
    }
    sm[g][l] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (l < s) sm[g][l] += sm[g][l + s];
      __syncthreads();
    }
    if (l == 0 && q < nsum) res[q] = sm[g][0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = halves == 2 ? res[2 * k] + res[2 * k + 1] : res[k];
#pragma unroll
    for (int k = 0; k < NV; k++) sums[k] = v[k];
    if (WHICH != 0) {
      BicgState s = *st;
      if (WHICH == 1) after_K1(s, v);
      if (WHICH == 3) after_K3(s, v, v[2]);
      if (WHICH == 4) {
        after_K4(s, v, v[2]);
        if (hist && s.it < hist_len) hist[s.it] = v[2];
      }
      *st = s;
    }
  }
}

static void destroy(tmhip_ctx *ctx) {
  Work *w = (Work *)ctx->bicg;
  if (!w) return;
  for (int k = 0; k < 2; k++) for (int i = 0; i < 6; i++) tmhip_field_free(ctx, w->f[k][i]);
  if (w->st) (void)hipFree(w->st);
  if (w->partials) (void)hipFree(w->partials);
  if (w->sums) (void)hipFree(w->sums);
  if (w->sums_host) (void)hipHostFree(w->sums_host);
  if (w->hist) (void)hipFree(w->hist);
  delete w;
  ctx->bicg = nullptr;
}

// the state, the block sums and -- fields true -- the six work fields of `kind`, on first use
static int work(tmhip_ctx *ctx, int kind, bool fields, Work **out) {
  TMHIP_CHECK(hipSetDevice(ctx->device));
  Work *w = (Work *)ctx->bicg;
  if (!w) {
    w = new (std::nothrow) Work();
    if (!w) TMHIP_FAIL("out of host memory");
    memset(w, 0, sizeof(*w));
    ctx->bicg = w;
    TMHIP_CHECK(hipMalloc((void **)&w->st, 2 * sizeof(BicgState)));
    TMHIP_CHECK(hipMemsetAsync(w->st, 0, 2 * sizeof(BicgState), ctx->stream));
    TMHIP_CHECK(hipMalloc((void **)&w->partials, (size_t)3 * 24 * la_grid(ctx->Vh).x * sizeof(double)));
    TMHIP_CHECK(hipMalloc((void **)&w->sums, 3 * sizeof(double)));
    TMHIP_CHECK(hipHostMalloc((void **)&w->sums_host, 3 * sizeof(double)));
  }
  if (fields)
    for (int i = 0; i < 6; i++)
      if (!w->f[kind][i] && tmhip_field_alloc(ctx, kind, &w->f[kind][i])) return 1;
  *out = w;
  return 0;
}

// the launch shape of fields of one kind: planes, sites per plane, block sums per (value, half)
struct Shape { int planes, n, halves, per; dim3 grid; };
static int shape_of(tmhip_ctx *ctx, const char *who, int N, int nf, tmhip_field *const *f, Shape *s) {
  for (int i = 0; i < nf; i++) {
    if (!f[i]) TMHIP_FAIL("%s: null field", who);
    if (f[i]->prec) TMHIP_FAIL("%s: fp64 fields only (fp32 is not built)", who);
    if (f[i]->kind != f[0]->kind || f[i]->ns != f[0]->ns) TMHIP_FAIL("%s: the fields must be of one kind", who);
  }
  const bool full = f[0]->kind == TMHIP_FIELD_FULL;
  if (N != (full ? ctx->V : ctx->Vh)) TMHIP_FAIL("%s: N = %d, but %s fields hold %d sites", who, N, full ? "FULL" : "EO", full ? ctx->V : ctx->Vh);
  s->planes = full ? 24 : 12; s->n = ctx->Vh; s->halves = full ? 2 : 1;
  s->grid = dim3(la_grid(ctx->Vh).x, s->planes);
  s->per = 12 * (int)s->grid.x;
  return 0;
}

// ---- the singles on fields of either kind: a FULL field is its two halves, one call each, sums added even first
static inline tmhip_field *part(tmhip_field *f, int h) { return f->kind == TMHIP_FIELD_FULL ? f->half[h] : f; }
static int s_assign(tmhip_ctx *c, const Shape &sh, tmhip_field *R, tmhip_field *S) {
  for (int h = 0; h < sh.halves; h++) if (tmhip_assign(c, part(R, h), part(S, h), sh.n)) return 1;
  return 0;
}
static int s_diff(tmhip_ctx *c, const Shape &sh, tmhip_field *Q, tmhip_field *R, tmhip_field *S) {
  for (int h = 0; h < sh.halves; h++) if (tmhip_diff(c, part(Q, h), part(R, h), part(S, h), sh.n)) return 1;
  return 0;
}
static int s_assign_diff_mul(tmhip_ctx *c, const Shape &sh, tmhip_field *R, tmhip_field *S, const double z[2]) {
  for (int h = 0; h < sh.halves; h++) if (tmhip_assign_diff_mul(c, part(R, h), part(S, h), z[0], z[1], sh.n)) return 1;
  return 0;
}
static int s_scalar_prod(tmhip_ctx *c, const Shape &sh, tmhip_field *S, tmhip_field *R, double out[2]) {
  out[0] = out[1] = 0.0;
  for (int h = 0; h < sh.halves; h++) {
    double r[2];
    if (tmhip_scalar_prod(c, part(S, h), part(R, h), sh.n, 1, r)) return 1;
    out[0] += r[0]; out[1] += r[1];
  }
  return 0;
}
static int s_square_norm(tmhip_ctx *c, const Shape &sh, tmhip_field *P, double *out) {
  *out = 0.0;
  for (int h = 0; h < sh.halves; h++) {
    double r;
    if (tmhip_square_norm(c, part(P, h), sh.n, 1, &r)) return 1;
    *out += r;
  }
  return 0;
}

// "bicg_fused" 0: the reference's statement sequence on the singles, one host round trip per scalar
static int solve_singles(tmhip_ctx *ctx, const Shape &sh, Work *w, BicgState &h, tmhip_field *P, int N, int op, double *res_hist, int hist_len) {
  tmhip_field **f = w->f[P->kind];
  tmhip_field *hatr = f[0], *r = f[1], *v = f[2], *p = f[3], *s = f[4], *t = f[5];
  for (int i = 0; i < h.max_iter; i++) {
    double err, denom[2], ts[2], tt, rho1[2];
    if (s_square_norm(ctx, sh, r, &err)) return 1;
    if (res_hist && i < hist_len) res_hist[i] = err;
    if (converged(err, h.eps_sq, h.squarenorm, h.rel_prec) && i > 0) { h.done = 1; h.iters = i; return 0; }
    if (tmhip_apply_op(ctx, op, v, p)) return 1;
    if (s_scalar_prod(ctx, sh, hatr, v, denom)) return 1;
    after_K1(h, denom);
    if (s_assign(ctx, sh, s, r) || s_assign_diff_mul(ctx, sh, s, v, h.alpha)) return 1;
    if (tmhip_apply_op(ctx, op, t, s)) return 1;
    if (s_scalar_prod(ctx, sh, t, s, ts) || s_square_norm(ctx, sh, t, &tt)) return 1;
    after_K3(h, ts, tt);
    if (tmhip_assign_add_mul_add_mul(ctx, P, p, s, h.alpha[0], h.alpha[1], h.omega[0], h.omega[1], N)) return 1;
    if (s_assign(ctx, sh, r, s) || s_assign_diff_mul(ctx, sh, r, t, h.omega)) return 1;
    if (s_scalar_prod(ctx, sh, hatr, r, rho1)) return 1;
    if (fabs(rho1[0]) < 1.e-25 && fabs(rho1[1]) < 1.e-25) { h.it = i + 1; h.iters = -1; return 0; }
    double nom[2], den[2];
    cmulh(h.alpha, rho1, nom);
    cmulh(h.omega, h.rho0, den);
    cdiv(nom, den, h.beta);
    if (tmhip_assign_mul_bra_add_mul_ket_add(ctx, p, v, r, h.nomega[0], h.nomega[1], h.beta[0], h.beta[1], N)) return 1;
    h.rho0[0] = rho1[0]; h.rho0[1] = rho1[1];
    h.it = i + 1;
  }
  if (res_hist && h.max_iter > 0 && h.max_iter < hist_len && s_square_norm(ctx, sh, r, &res_hist[h.max_iter])) return 1;   // as the fused path: |r|^2 after the last iteration
  h.iters = -1;
  return 0;
}

static int enqueue_iteration(tmhip_ctx *ctx, const Shape &sh, Work *w, tmhip_field *P, int op) {
  tmhip_field **f = w->f[P->kind];
  v2d *hatr = f[0]->d, *r = f[1]->d, *v = f[2]->d, *p = f[3]->d, *s = f[4]->d, *t = f[5]->d;
  const int ns = P->ns;
  BicgState *st = w->st;
  const dim3 bs(LA_BS);
  if (tmhip_apply_op(ctx, op, f[2], f[3])) return 1;
  hipLaunchKernelGGL(dot_kernel<false>, sh.grid, bs, 0, ctx->stream, (const v2d *)hatr, (const v2d *)v, ns, sh.n, w->partials, (const BicgState *)st);
  hipLaunchKernelGGL(sum_scalar_kernel<1>, dim3(1), dim3(1024), 0, ctx->stream, (const double *)w->partials, sh.per, sh.halves, st, w->sums, w->hist, w->hist_len);
  hipLaunchKernelGGL(sub_kernel, sh.grid, bs, 0, ctx->stream, s, (const v2d *)r, (const v2d *)v, ns, sh.n, (const BicgState *)st);
  if (tmhip_apply_op(ctx, op, f[5], f[4])) return 1;
  hipLaunchKernelGGL(dot_kernel<true>, sh.grid, bs, 0, ctx->stream, (const v2d *)t, (const v2d *)s, ns, sh.n, w->partials, (const BicgState *)st);
  hipLaunchKernelGGL(sum_scalar_kernel<3>, dim3(1), dim3(1024), 0, ctx->stream, (const double *)w->partials, sh.per, sh.halves, st, w->sums, w->hist, w->hist_len);
  hipLaunchKernelGGL(update_kernel, sh.grid, bs, 0, ctx->stream, P->d, r, (const v2d *)p, (const v2d *)s, (const v2d *)t, (const v2d *)hatr, ns, sh.n,
                     w->partials, (const BicgState *)st);
  hipLaunchKernelGGL(sum_scalar_kernel<4>, dim3(1), dim3(1024), 0, ctx->stream, (const double *)w->partials, sh.per, sh.halves, st, w->sums, w->hist, w->hist_len);
  hipLaunchKernelGGL(dir_kernel, sh.grid, bs, 0, ctx->stream, p, (const v2d *)v, (const v2d *)r, ns, sh.n, (const BicgState *)st);
  return 0;
}

static int refuse_split(tmhip_ctx *ctx, const char *who) {
  if (ctx->g.nproc_t > 1 || ctx->loopback) TMHIP_FAIL("%s: T-split ranks (and their loopback rehearsal) are not built: the sums are rank-local", who);
  return 0;
}

// the second state block with the host's scalars in it, for the entry points that run one kernel of the iteration alone
static int host_scalars(tmhip_ctx *ctx, Work *w, const double *alpha, const double *omega, const double *beta) {
  BicgState h;
  memset(&h, 0, sizeof(h));
  if (alpha) { h.alpha[0] = alpha[0]; h.alpha[1] = alpha[1]; }
  if (omega) { h.omega[0] = omega[0]; h.omega[1] = omega[1]; h.nomega[0] = -omega[0]; h.nomega[1] = -omega[1]; }
  if (beta) { h.beta[0] = beta[0]; h.beta[1] = beta[1]; }
  TMHIP_CHECK(hipMemcpyAsync(w->st + 1, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));   // h leaves scope
  return 0;
}
static int sums_to_host(tmhip_ctx *ctx, Work *w, const Shape &sh, double out[3]) {
  hipLaunchKernelGGL(sum_scalar_kernel<0>, dim3(1), dim3(1024), 0, ctx->stream, (const double *)w->partials, sh.per, sh.halves, w->st + 1, w->sums,
                     (double *)nullptr, 0);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(w->sums_host, w->sums, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 3; k++) out[k] = w->sums_host[k];
  return tmhip_check_async_error(ctx);
}

}  // namespace bicghip

using namespace bicghip;

void tmhip_bicg_destroy(tmhip_ctx *ctx) { bicghip::destroy(ctx); }

extern "C" {

int tmhip_bicg_update(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *r, tmhip_field *p, tmhip_field *s, tmhip_field *t, tmhip_field *hatr,
                      const double alpha[2], const double omega[2], int N, double out[3]) {
  tmhip_field *f[6] = {P, r, p, s, t, hatr};
  Shape sh;
  Work *w;
  if (!alpha || !omega || !out) TMHIP_FAIL("bicg_update: null argument");
  if (refuse_split(ctx, "bicg_update") || shape_of(ctx, "bicg_update", N, 6, f, &sh)) return 1;
  for (int i = 0; i < 2; i++) for (int j = 0; j < 6; j++) if (j != i && f[j]->d == f[i]->d) TMHIP_FAIL("bicg_update: P and r may not be any other field of the call");
  if (work(ctx, P->kind, false, &w) || host_scalars(ctx, w, alpha, omega, nullptr)) return 1;
  hipLaunchKernelGGL(update_kernel, sh.grid, dim3(LA_BS), 0, ctx->stream, P->d, r->d, (const v2d *)p->d, (const v2d *)s->d, (const v2d *)t->d,
                     (const v2d *)hatr->d, P->ns, sh.n, w->partials, (const BicgState *)(w->st + 1));
  return sums_to_host(ctx, w, sh, out);
}

int tmhip_bicg_pair_dot(tmhip_ctx *ctx, tmhip_field *t, tmhip_field *s, int N, double out[3]) {
  tmhip_field *f[2] = {t, s};
  Shape sh;
  Work *w;
  if (!out) TMHIP_FAIL("bicg_pair_dot: null argument");
  if (refuse_split(ctx, "bicg_pair_dot") || shape_of(ctx, "bicg_pair_dot", N, 2, f, &sh)) return 1;
  if (work(ctx, t->kind, false, &w) || host_scalars(ctx, w, nullptr, nullptr, nullptr)) return 1;
  hipLaunchKernelGGL(dot_kernel<true>, sh.grid, dim3(LA_BS), 0, ctx->stream, (const v2d *)t->d, (const v2d *)s->d, t->ns, sh.n, w->partials,
                     (const BicgState *)(w->st + 1));
  return sums_to_host(ctx, w, sh, out);
}

int tmhip_bicg_sub(tmhip_ctx *ctx, tmhip_field *s, tmhip_field *r, tmhip_field *v, const double alpha[2], int N) {
  tmhip_field *f[3] = {s, r, v};
  Shape sh;
  Work *w;
  if (!alpha) TMHIP_FAIL("bicg_sub: null argument");
  if (refuse_split(ctx, "bicg_sub") || shape_of(ctx, "bicg_sub", N, 3, f, &sh)) return 1;
  if (s->d == r->d || s->d == v->d) TMHIP_FAIL("bicg_sub: s may not be r or v");
  if (work(ctx, s->kind, false, &w) || host_scalars(ctx, w, alpha, nullptr, nullptr)) return 1;
  hipLaunchKernelGGL(sub_kernel, sh.grid, dim3(LA_BS), 0, ctx->stream, s->d, (const v2d *)r->d, (const v2d *)v->d, s->ns, sh.n, (const BicgState *)(w->st + 1));
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_bicg_dir(tmhip_ctx *ctx, tmhip_field *p, tmhip_field *v, tmhip_field *r, const double omega[2], const double beta[2], int N) {
  tmhip_field *f[3] = {p, v, r};
  Shape sh;
  Work *w;
  if (!omega || !beta) TMHIP_FAIL("bicg_dir: null argument");
  if (refuse_split(ctx, "bicg_dir") || shape_of(ctx, "bicg_dir", N, 3, f, &sh)) return 1;
  if (p->d == v->d || p->d == r->d) TMHIP_FAIL("bicg_dir: p may not be v or r");
  if (work(ctx, p->kind, false, &w) || host_scalars(ctx, w, nullptr, omega, beta)) return 1;
  hipLaunchKernelGGL(dir_kernel, sh.grid, dim3(LA_BS), 0, ctx->stream, p->d, (const v2d *)v->d, (const v2d *)r->d, p->ns, sh.n, (const BicgState *)(w->st + 1));
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_bicgstab_complex(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, int max_iter, double eps_sq, int rel_prec, int N, int op, int *iters,
                           double *res_hist, int hist_len) {
  const char *who = "bicgstab_complex";
  if (!iters) TMHIP_FAIL("%s: null argument", who);
  if (refuse_split(ctx, who)) return 1;
  if (!P || !Q || P->kind != Q->kind) TMHIP_FAIL("%s needs two fields of one kind", who);
  if (tmhip_op_check(ctx, who, TMHIP_S_BICG, op, P->kind)) return 1;
  const int kind = P->kind;
  tmhip_field *pq[2] = {P, Q};
  Shape sh;
  if (shape_of(ctx, who, N, 2, pq, &sh)) return 1;
  if (P->d == Q->d) TMHIP_FAIL("%s: P and Q must differ", who);
  if (!ctx->gauge_set) TMHIP_FAIL("%s called before tmhip_set_gauge", who);
  Work *w;
  if (work(ctx, kind, true, &w)) return 1;
  if (max_iter + 1 > w->hist_len) {
    if (w->hist) TMHIP_CHECK(hipFree(w->hist));
    w->hist = nullptr; w->hist_len = 0;
    TMHIP_CHECK(hipMalloc((void **)&w->hist, sizeof(double) * ((size_t)max_iter + 1)));
    w->hist_len = max_iter + 1;
  }
  tmhip_field **f = w->f[kind];
  tmhip_field *hatr = f[0], *r = f[1], *p = f[3];
  // :72-77, once per solve: host-visible scalars are fine here
  BicgState h;
  memset(&h, 0, sizeof(h));
  h.eps_sq = eps_sq; h.rel_prec = rel_prec; h.max_iter = max_iter;
  if (tmhip_apply_op(ctx, op, r, P)) return 1;
  if (s_diff(ctx, sh, p, Q, r) || s_assign(ctx, sh, r, p) || s_assign(ctx, sh, hatr, p)) return 1;
  if (s_scalar_prod(ctx, sh, hatr, r, h.rho0) || s_square_norm(ctx, sh, Q, &h.squarenorm)) return 1;
  if (!ctx->opt_bicg_fused) {
    if (solve_singles(ctx, sh, w, h, P, N, op, res_hist, hist_len)) return 1;
    *iters = h.iters;
    return 0;
  }
  if (s_square_norm(ctx, sh, r, &h.err)) return 1;   // :80 of the first iteration (the later ones take it from K4)
  if (max_iter <= 0) { *iters = -1; return 0; }
  TMHIP_CHECK(hipMemcpyAsync(w->st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipMemcpyAsync(w->hist, &h.err, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  const int batch = ctx->opt_cg_batch > 0 ? ctx->opt_cg_batch : 4;
  const double target = rel_prec == 1 ? eps_sq * h.squarenorm : eps_sq;
  if (tmhip_poll_loop(ctx, max_iter, true, batch, 1.0e3 * target, &w->st->done, &w->st->err, 0, true,
                      [&](int) { return enqueue_iteration(ctx, sh, w, P, op); })) return 1;
  TMHIP_CHECK(hipMemcpyAsync(&h, w->st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *iters = h.done ? h.iters : -1;
  if (res_hist && hist_len > 0) {
    const int n = h.it + 1 < hist_len ? h.it + 1 : hist_len;
    TMHIP_CHECK(hipMemcpy(res_hist, w->hist, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // extern "C"
