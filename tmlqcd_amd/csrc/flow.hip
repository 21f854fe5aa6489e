// Wilson gradient flow (meas/gradient_flow.c) and the clover field-strength observables
// (meas/measure_clover_field_strength_observables.c) on the device-resident links, fp64, unsplit lattices.
//   tmhip_flow_begin / _step / _observables / _download / _end   step_gradient_flow (gradient_flow.c:52-130) on two private link buffers
//   tmhip_gradient_flow                                          the measurement loop of gradient_flow_measurement (:172-222)
//   tmhip_measure_field_strength                                 E and Q of the resident links
// The resident links ctx->gauge_raw are only ever read: flow_begin copies them into W0, and a step runs its three Runge-Kutta stages
// out of place W0 -> W1 -> W0 -> W1 (a stage reads the neighbours of its source field), after which the two buffers swap roles.
// Stage kernel: the block shape of gauge_force_kernel (gauge.hip) -- 256 threads = 64 lexicographic sites x the four directions, the
// direction wave-uniform -- one thread per link: plaquette staples of the source field (gauge_common.h), staple U^dagger, projection,
// the Z recurrence, the second projection, the Cayley-Hamilton exponential (matrix_utils.c:45-115) and U' = exp U.  Z is traceless
// anti-hermitian after every operation of the recurrence, element for element, so it is kept as NINE reals per link (72 bytes: the
// imaginary diagonal and c01, c02, c12), in planes [9][4][V] so that a wave's accesses are contiguous; nothing a thread writes is
// read by another thread of the same launch.
// Field-strength kernel: one thread per site.  A clover leaf is four closed four-link paths (path_product, rolled) summed and
// projected to nine reals; the planes are walked in the three pairs a Levi-Civita term of Q joins, two leaves live at a time.
#include "gauge_common.h"

namespace flowhip {
using namespace gaugehip;

struct FlowState {
  v2d *w[2];     // link buffers [V][4][9], w[cur] holds the flowed links
  double *z;     // [9][4][V]
  int cur;
};

// project_traceless_antiherm (matrix_utils.c:117-137) into nine reals: a[0..2] = Im c00, c11, c22; (a[3], a[4]) = c01, (a[5], a[6]) = c02,
// (a[7], a[8]) = c12; c10 = -conj(c01) etc. are implied.  Note the factor 0.5 and that the diagonal keeps its imaginary part only.
__device__ __forceinline__ void project_tah(double (&a)[9], const cd (&m)[9]) {
  const double tr = (1.00 / 3.00) * (m[0].y + m[4].y + m[8].y);
  a[0] = m[0].y - tr;
  a[1] = m[4].y - tr;
  a[2] = m[8].y - tr;
  a[3] = (m[1].x - m[3].x) * 0.50;
  a[4] = (m[1].y + m[3].y) * 0.50;
  a[5] = (m[2].x - m[6].x) * 0.50;
  a[6] = (m[2].y + m[6].y) * 0.50;
  a[7] = (m[5].x - m[7].x) * 0.50;
  a[8] = (m[5].y + m[7].y) * 0.50;
}
// the same projection applied to a matrix that is anti-hermitian already: the off-diagonal (c01 + c01) 0.5 is exact, the trace is not
__device__ __forceinline__ void project_tah9(double (&a)[9]) {
  const double tr = (1.00 / 3.00) * (a[0] + a[1] + a[2]);
  a[0] -= tr;
  a[1] -= tr;
  a[2] -= tr;
}
__device__ __forceinline__ void expand_tah(cd (&m)[9], const double (&a)[9]) {
  m[0] = cd{0.0, a[0]}; m[1] = cd{a[3], a[4]};  m[2] = cd{a[5], a[6]};
  m[3] = cd{-a[3], a[4]}; m[4] = cd{0.0, a[1]}; m[5] = cd{a[7], a[8]};
  m[6] = cd{-a[5], a[6]}; m[7] = cd{-a[7], a[8]}; m[8] = cd{0.0, a[2]};
}
__device__ __forceinline__ double re_mul(cd a, cd b) { return a.x * b.x - a.y * b.y; }

// cayley_hamilton_exponent (matrix_utils.c:45-115), formula by formula, and exponent_from_coefficients (:36-43)
__device__ __forceinline__ void cayley_hamilton_exponent(cd (&out)[9], const cd (&A)[9]) {
  const double fac_1_3 = 1 / 3.0;
  // c0 = Re(I det A), c1 = -0.5 Re tr(A A)
  const cd det = g_cmul(A[0], g_cmul(A[4], A[8]) - g_cmul(A[5], A[7])) + g_cmul(A[1], g_cmul(A[5], A[6]) - g_cmul(A[3], A[8])) +
                 g_cmul(A[2], g_cmul(A[3], A[7]) - g_cmul(A[4], A[6]));
  double c0 = -det.y;
  const double c1 = -0.5 * (re_mul(A[0], A[0]) + re_mul(A[1], A[3]) + re_mul(A[2], A[6]) + re_mul(A[3], A[1]) + re_mul(A[4], A[4]) +
                            re_mul(A[5], A[7]) + re_mul(A[6], A[2]) + re_mul(A[7], A[5]) + re_mul(A[8], A[8]));
  if (c0 == 0 && c1 == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) out[e] = cd{(e & 3) == 0 ? 1.0 : 0.0, 0.0};
    return;
  }
  const bool c0_negative = c0 < 0;
  c0 = fabs(c0);
  const double c0max = 2.0 * pow(fac_1_3 * c1, 1.5);
  const double theta_3 = fac_1_3 * acos(fmin(c0 / c0max, 1.0));
  const double u = sqrt(fac_1_3 * c1) * cos(theta_3);
  const double w = sqrt(c1) * sin(theta_3);
  const cd ma = cd{cos(2 * u), sin(2 * u)};     // cexp(2 I u)
  const cd mb = cd{cos(u), -sin(u)};            // cexp(-I u)
  const double cw = cos(w);
  const double u2 = u * u;
  const double w2 = w * w;
  const double xi0 = (w > 0.05) ? (sin(w) / w) : 1 - 0.16666666666666667 * w2 * (1 - 0.05 * w2 * (1 - 0.023809523809523808 * w2));
  const double divisor = 1.0 / (9.0 * u2 - w2);
  const double uw = u * u - w * w;
  cd f0 = g_cmul(mb, cd{8 * u * u * cw, 2 * u * (3 * u * u + w * w) * xi0});
  f0 = cd{divisor * (ma.x * uw + f0.x), divisor * (ma.y * uw + f0.y)};
  cd f1 = g_cmul(mb, cd{(3 * u * u - w * w) * xi0, 2 * u * cw});
  f1 = cd{divisor * (2 * u * ma.y + f1.x), divisor * (-2 * u * ma.x + f1.y)};
  cd f2 = g_cmul(mb, cd{cw, 3 * u * xi0});
  f2 = cd{divisor * (f2.x - ma.x), divisor * (f2.y - ma.y)};
  if (c0_negative) { f0.y = -f0.y; f1.y = -f1.y; f2.y = -f2.y; }
  cd tmp[9];
#pragma unroll
  for (int e = 0; e < 9; e++) tmp[e] = g_cmul(f2, A[e]);
  tmp[0] += f1; tmp[4] += f1; tmp[8] += f1;
  mm(out, tmp, A);
  out[0] += f0; out[4] += f0; out[8] += f0;
}

// One Runge-Kutta stage of step_gradient_flow (gradient_flow.c:80-109) for the link (ix, mu): src -> dst, Z updated in place by its owner
template <int STAGE>
__global__ __launch_bounds__(256, 2) void flow_stage_kernel(const v2d *__restrict__ src, v2d *__restrict__ dst, double *__restrict__ Z, GaugeGeom g, double eps) {
  const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mu = threadIdx.x >> 6;
  if (ix >= g.V) return;
  const Site s = g_site(g, ix);
  double p[9];
  {
    cd u[9], v[9], w[9];
    plaquette_staples(v, src, g, s, mu, 1.0, 1.0);
    g_load(u, src, g, s, mu);
    mmd(w, v, u);                       // staple U^dagger: "usually we dagger the staples, but the sign convention seems to require this"
    project_tah(p, w);
  }
  const double zfac[5] = {1, (8.0) / (9.0), (-17.0) / (36.0), (3.0) / (4.0), -1};
  const double zepsfac[3] = {0.25, 1, 1};
  double *z = Z + (size_t)mu * g.V + ix;
  const size_t zs = (size_t)4 * g.V;
  if (STAGE == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) p[e] = eps * p[e];
  } else {
    const double a = eps * zfac[2 * STAGE - 1];
#pragma unroll
    for (int e = 0; e < 9; e++) {
      double t = a * p[e];
      t += zfac[2 * STAGE] * z[e * zs];
      p[e] = t;
    }
  }
  if (STAGE < 2) {                      // the next step's first stage overwrites Z without reading it
#pragma unroll
    for (int e = 0; e < 9; e++) z[e * zs] = p[e];
  }
#pragma unroll
  for (int e = 0; e < 9; e++) p[e] = zepsfac[STAGE] * p[e];
  project_tah9(p);
  cd A[9], ex[9], u[9], r[9];
  expand_tah(A, p);
  cayley_hamilton_exponent(ex, A);
  g_load(u, src, g, s, mu);
  mm(r, ex, u);
  v2d *o = dst + ((size_t)ix * 4 + mu) * 9;
#pragma unroll
  for (int e = 0; e < 9; e++) o[e] = r[e];
}

// The clover leaf of the plane (k, l) at s: the four plaquettes around s in the order of
// measure_clover_field_strength_observables.c:135-162, each a closed path from s (mu = k, nu = l in the step codes), summed and projected
__device__ __forceinline__ void clover_leaf(double (&a)[9], const v2d *__restrict__ raw, const GaugeGeom &g, Site s, int k, int l) {
  cd G[9];
#pragma unroll
  for (int e = 0; e < 9; e++) G[e] = cd{0.0, 0.0};
#pragma unroll 1
  for (int h = 0; h < 4; h++) {
    const unsigned code = h == 0 ? g_path(2, 0, 3, 1) : h == 1 ? g_path(0, 3, 1, 2) : h == 2 ? g_path(3, 1, 2, 0) : g_path(1, 2, 0, 3);
    cd acc[9];
    path_product<4>(acc, raw, g, s, k, l, code);
#pragma unroll
    for (int e = 0; e < 9; e++) G[e] += acc[e];
  }
  project_tah(a, G);
}
// Re tr(A B) of two projected leaves, the nine terms in the order of _trace_su3_times_su3 (su3.h:667-676)
__device__ __forceinline__ double tr_leaves(const double (&a)[9], const double (&b)[9]) {
  const double o01 = -(a[3] * b[3] + a[4] * b[4]), o02 = -(a[5] * b[5] + a[6] * b[6]), o12 = -(a[7] * b[7] + a[8] * b[8]);
  double x = -(a[0] * b[0]);
  x += o01;
  x += o02;
  x += o01;
  x += -(a[1] * b[1]);
  x += o12;
  x += o02;
  x += o12;
  x += -(a[2] * b[2]);
  return x;
}

// partials[b] = block b's sum of tr(G_kl G_kl) over its sites and the six planes k < l, partials[nb + b] = its sum of the six surviving
// Levi-Civita terms of new_epsilon4() (tensors.h:65-92) in its order: +(01,23) -(02,13) +(03,12) +(12,03) -(13,02) +(23,01)
__global__ __launch_bounds__(256, 2) void field_strength_kernel(const v2d *__restrict__ raw, GaugeGeom g, double *__restrict__ partials, int nb) {
  const int ix = blockIdx.x * 256 + threadIdx.x;
  double E = 0.0, Q = 0.0;
  if (ix < g.V) {
    const Site s = g_site(g, ix);
    // Planes are taken in the pairs a Levi-Civita term joins -- (01, 23), (02, 13), (03, 12) -- in a rolled loop, so that two projected
    // leaves and one path product are live at a time (all six leaves unrolled: 256 VGPRs and 288 bytes of scratch).  The per-plane and
    // per-pair values are kept as scalars and added afterwards in the reference's order.
    double ea0 = 0.0, ea1 = 0.0, ea2 = 0.0, eb0 = 0.0, eb1 = 0.0, eb2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
#pragma unroll 1
    for (int p = 0; p < 3; p++) {
      double a[9], b[9];
      clover_leaf(a, raw, g, s, 0, p + 1);
      clover_leaf(b, raw, g, s, p == 0 ? 2 : 1, p == 2 ? 2 : 3);
      const double ea = tr_leaves(a, a), eb = tr_leaves(b, b), q = tr_leaves(a, b);   // tr_leaves(a, b) == tr_leaves(b, a) bit for bit
      ea0 = p == 0 ? ea : ea0; ea1 = p == 1 ? ea : ea1; ea2 = p == 2 ? ea : ea2;
      eb0 = p == 0 ? eb : eb0; eb1 = p == 1 ? eb : eb1; eb2 = p == 2 ? eb : eb2;
      q0 = p == 0 ? q : q0; q1 = p == 1 ? q : q1; q2 = p == 2 ? q : q2;
    }
    E += ea0; E += ea1; E += ea2; E += eb2; E += eb1; E += eb0;      // planes 01, 02, 03, 12, 13, 23
    Q += q0; Q += -q1; Q += q2; Q += q2; Q += -q1; Q += q0;
  }
  // the library's reproducible reduction, for both sums at once
  __shared__ double wsum[8];
  E = tmhip_wave_sum(E);
  Q = tmhip_wave_sum(Q);
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = E; wsum[4 + (threadIdx.x >> 6)] = Q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    partials[nb + blockIdx.x] = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
  }
}
// block b adds up partials[b nb .. (b + 1) nb) in the fixed order of tmhip_block_sum256
__global__ __launch_bounds__(256) void field_strength_final_kernel(const double *__restrict__ partials, int nb, double *__restrict__ out) {
  __shared__ double wsum[4];
  const double v = tmhip_block_sum256(partials + (size_t)blockIdx.x * nb, nb, wsum);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

static int flow_ready(tmhip_ctx *ctx, const char *who) {
  if (gauge_ready(ctx, who, false)) return 1;
  if (ctx->g.nproc_t > 1) TMHIP_FAIL("%s: a T-split rank would need its link halo refreshed after every stage; not available with nproc_t > 1", who);
  return 0;
}
static int flow_live(tmhip_ctx *ctx, const char *who, FlowState **st) {
  if (flow_ready(ctx, who)) return 1;
  if (!ctx->flow) TMHIP_FAIL("%s: no flow in progress (tmhip_flow_begin first)", who);
  *st = (FlowState *)ctx->flow;
  return 0;
}

// E and Q of a link field [V][4][9], normalised as measure_clover_field_strength_observables.c:68-72, :223-224 with g_nproc = 1
static int field_strength(tmhip_ctx *ctx, const v2d *links, double *E, double *Q) {
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const int nb = (ctx->V + 255) / 256;
  if (2 * nb > ctx->max_partials) TMHIP_FAIL("field strength: partials buffer too small");
  const GaugeGeom g = gauge_geom(ctx);
  hipLaunchKernelGGL(field_strength_kernel, dim3(nb), dim3(256), 0, ctx->stream, links, g, ctx->partials, nb);
  hipLaunchKernelGGL(field_strength_final_kernel, dim3(2), dim3(256), 0, ctx->stream, (const double *)ctx->partials, nb, ctx->result_dev);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(ctx->result_host, ctx->result_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  const double energy_density_normalization = -4 / (4 * 16.0 * ctx->V);
  const double topo_charge_normalization = -1 / (4 * 32.0 * M_PI * M_PI);
  *E = energy_density_normalization * ctx->result_host[0];
  *Q = topo_charge_normalization * ctx->result_host[1];
  return 0;
}

static int flow_step(tmhip_ctx *ctx, FlowState *st, double eps) {
  TMHIP_CHECK(hipSetDevice(ctx->device));
  const GaugeGeom g = gauge_geom(ctx);
  const dim3 grid((ctx->V + 63) / 64);
  v2d *a = st->w[st->cur], *b = st->w[st->cur ^ 1];
  hipLaunchKernelGGL(flow_stage_kernel<0>, grid, dim3(256), 0, ctx->stream, (const v2d *)a, b, st->z, g, eps);
  hipLaunchKernelGGL(flow_stage_kernel<1>, grid, dim3(256), 0, ctx->stream, (const v2d *)b, a, st->z, g, eps);
  hipLaunchKernelGGL(flow_stage_kernel<2>, grid, dim3(256), 0, ctx->stream, (const v2d *)a, b, st->z, g, eps);
  TMHIP_CHECK(hipGetLastError());
  st->cur ^= 1;
  return 0;
}

static int flow_observables(tmhip_ctx *ctx, FlowState *st, double *P, double *E, double *Q) {
  double p = 0.0;
  if (gauge_sum(ctx, st->w[st->cur], false, 1.0, 1.0, &p)) return 1;
  *P = p / (6.0 * ctx->V);
  return field_strength(ctx, st->w[st->cur], E, Q);
}
}  // namespace flowhip
using namespace flowhip;

void tmhip_flow_destroy(tmhip_ctx *ctx) {
  FlowState *st = (FlowState *)ctx->flow;
  if (!st) return;
  for (int i = 0; i < 2; i++) if (st->w[i]) (void)hipFree(st->w[i]);
  if (st->z) (void)hipFree(st->z);
  delete st;
  ctx->flow = nullptr;
}

extern "C" {

int tmhip_measure_field_strength(tmhip_ctx *ctx, double *E, double *Q) {
  if (!E || !Q) TMHIP_FAIL("tmhip_measure_field_strength: null argument");
  if (flow_ready(ctx, "tmhip_measure_field_strength")) return 1;
  return field_strength(ctx, (const v2d *)ctx->gauge_raw, E, Q);
}

int tmhip_flow_begin(tmhip_ctx *ctx) {
  if (flow_ready(ctx, "tmhip_flow_begin")) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  FlowState *st = (FlowState *)ctx->flow;
  if (!st) {
    st = new (std::nothrow) FlowState();
    if (!st) TMHIP_FAIL("tmhip_flow_begin: out of host memory");
    st->w[0] = st->w[1] = nullptr; st->z = nullptr;
    ctx->flow = st;
    const size_t lb = (size_t)ctx->V * 36 * sizeof(v2d);
    for (int i = 0; i < 2; i++)
      if (hipMalloc((void **)&st->w[i], lb) != hipSuccess) { tmhip_flow_destroy(ctx); TMHIP_FAIL("tmhip_flow_begin: no memory for the flow buffers (2 x %zu bytes of links)", lb); }
    if (hipMalloc((void **)&st->z, (size_t)ctx->V * 36 * sizeof(double)) != hipSuccess) { tmhip_flow_destroy(ctx); TMHIP_FAIL("tmhip_flow_begin: no memory for Z"); }
  }
  st->cur = 0;
  TMHIP_CHECK(hipMemcpyAsync(st->w[0], ctx->gauge_raw, (size_t)ctx->V * 36 * sizeof(v2d), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

int tmhip_flow_step(tmhip_ctx *ctx, double eps) {
  FlowState *st = nullptr;
  if (flow_live(ctx, "tmhip_flow_step", &st)) return 1;
  return flow_step(ctx, st, eps);
}

int tmhip_flow_observables(tmhip_ctx *ctx, double *P, double *E, double *Q) {
  if (!P || !E || !Q) TMHIP_FAIL("tmhip_flow_observables: null argument");
  FlowState *st = nullptr;
  if (flow_live(ctx, "tmhip_flow_observables", &st)) return 1;
  return flow_observables(ctx, st, P, E, Q);
}

int tmhip_flow_download(tmhip_ctx *ctx, void *host_gauge) {
  if (!host_gauge) TMHIP_FAIL("tmhip_flow_download: null argument");
  FlowState *st = nullptr;
  if (flow_live(ctx, "tmhip_flow_download", &st)) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  TMHIP_CHECK(hipMemcpyAsync(host_gauge, st->w[st->cur], (size_t)ctx->V * 36 * sizeof(v2d), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tmhip_flow_end(tmhip_ctx *ctx) {
  if (flow_ready(ctx, "tmhip_flow_end")) return 1;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  tmhip_flow_destroy(ctx);
  return 0;
}

/* gradient_flow.c:172-222: measure at t = 0, then pairs of steps with one row at the odd step */
int tmhip_gradient_flow(tmhip_ctx *ctx, double eps, double tmax, int max_rows, double *rows, int *nrows) {
  if (!nrows || max_rows < 0 || (max_rows > 0 && !rows)) TMHIP_FAIL("tmhip_gradient_flow: bad arguments");
  *nrows = 0;
  if (flow_ready(ctx, "tmhip_gradient_flow")) return 1;
  if (!(eps > 0.0)) TMHIP_FAIL("tmhip_gradient_flow: eps = %g, the loop would never reach tmax", eps);
  if (tmhip_flow_begin(ctx)) return 1;
  FlowState *st = (FlowState *)ctx->flow;
  double t[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0}, E[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0};
  int n = 0, rc = flow_observables(ctx, st, &P[2], &E[2], &Q[2]);
  while (!rc && t[1] < tmax) {
    if (n >= max_rows) {
      fprintf(stderr, "[tmlqcd_hip] tmhip_gradient_flow: more than max_rows = %d rows\n", max_rows);
      rc = 1;
      break;
    }
    t[0] = t[2]; E[0] = E[2]; Q[0] = Q[2]; P[0] = P[2];
    for (int step = 1; step < 3 && !rc; ++step) {
      t[step] = t[step - 1] + eps;
      rc = flow_step(ctx, st, eps) || flow_observables(ctx, st, &P[step], &E[step], &Q[step]);
    }
    if (rc) break;
    const double W = t[1] * t[1] * (2 * E[1] + t[1] * ((E[2] - E[0]) / (2 * eps)));
    const double tsqE = t[1] * t[1] * E[1];
    double *r = rows + (size_t)8 * n;
    r[0] = t[1]; r[1] = P[1]; r[2] = 36 * (1 - P[1]); r[3] = E[1]; r[4] = t[1] * t[1] * 36 * (1 - P[1]); r[5] = tsqE; r[6] = W; r[7] = Q[1];
    n++;
  }
  if (tmhip_flow_end(ctx)) return 1;
  if (rc) return 1;
  *nrows = n;
  return 0;
}

}  // extern "C"
