// Spinor linear algebra + site-diagonal twisted-mass operators on SoA device fields (gfx950).
//
// Reference semantics: linalg/{square_norm,scalar_prod_r,assign_add_mul_r,assign_mul_add_r,
// assign_mul_add_r_and_square,diff,assign}.c, gamma.c:77-98 and the site-diagonal ops of
// operator/tm_operators.c:587-858.  All are HBM-bound streams: 16 B/lane loads of one SoA
// plane, grid.y = the 12 (spin,colour) planes so no index arithmetic is needed.
//
// Reductions: per-thread partial -> 64-lane wavefront butterfly (__shfl_xor, lowered to
// DPP/ds_bpermute) -> LDS across the waves of the block -> one partial per block ->
// single-block fixed-order final pass (bitwise reproducible run to run; no atomics).
// The reference compensates a *sequential* sum with Kahan (square_norm.c:275-296); the
// pairwise tree used here has an error bound of O(log N) ulp, tighter than the
// sequential one, so no compensation is needed to stay within 1e-13 relative.
#include "tmhip_internal.h"
#include <type_traits>

__device__ __forceinline__ void block_reduce_store(double v, double *partials) {
  __shared__ double wsum[LA_BS / 64];
  v = tmhip_wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_BS / 64; k++) s += wsum[k];
    partials[blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(LA_BS) void sqnorm_kernel(const v2d *__restrict__ P, int ns, int N, double *partials) {
  const v2d *p = P + (size_t)blockIdx.y * ns;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) { const v2d a = p[i]; acc += a.x * a.x + a.y * a.y; }
  }
  block_reduce_store(acc, partials);
}

// Re <S,R> = sum Re(r * conj(s))   (scalar_prod_r.c:161-165)
__global__ __launch_bounds__(LA_BS) void dotr_kernel(const v2d *__restrict__ S, const v2d *__restrict__ R, int ns, int N,
                                                     double *partials) {
  const v2d *s = S + (size_t)blockIdx.y * ns, *r = R + (size_t)blockIdx.y * ns;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) { const v2d a = s[i], b = r[i]; acc += a.x * b.x + a.y * b.y; }
  }
  block_reduce_store(acc, partials);
}

// R = c R + S, returns |R|^2   (assign_mul_add_r_and_square.c:165-196)
__global__ __launch_bounds__(LA_BS) void xpay_sq_kernel(v2d *__restrict__ R, double c, const v2d *__restrict__ S, int ns, int N,
                                                        double *partials) {
  v2d *r = R + (size_t)blockIdx.y * ns;
  const v2d *s = S + (size_t)blockIdx.y * ns;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      v2d a = r[i];
      const v2d b = s[i];
      a = v2d{c * a.x + b.x, c * a.y + b.y};
      r[i] = a;
      acc += a.x * a.x + a.y * a.y;
    }
  }
  block_reduce_store(acc, partials);
}

__global__ __launch_bounds__(256) void reduce_final_kernel(const double *__restrict__ partials, int n, double *out) {
  __shared__ double sm[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partials[i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sm[0];
}

// MODE 0: P += c Q   1: R = c R + S   2: Q = R - S   3: R = S   4: Q = R + S   5: R = c S
template <int MODE>
__global__ __launch_bounds__(LA_BS) void stream_kernel(v2d *__restrict__ X, const v2d *__restrict__ Y, const v2d *__restrict__ Z,
                                                       double c, int ns, int N) {
  v2d *x = X + (size_t)blockIdx.y * ns;
  const v2d *y = Y + (size_t)blockIdx.y * ns;
  const v2d *z = Z ? Z + (size_t)blockIdx.y * ns : nullptr;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      if (MODE == 0) { const v2d a = x[i], b = y[i]; x[i] = v2d{a.x + c * b.x, a.y + c * b.y}; }
      if (MODE == 1) { const v2d a = x[i], b = y[i]; x[i] = v2d{c * a.x + b.x, c * a.y + b.y}; }
      if (MODE == 2) { x[i] = y[i] - z[i]; }
      if (MODE == 3) { x[i] = y[i]; }
      if (MODE == 4) { x[i] = y[i] + z[i]; }
      if (MODE == 5) { const v2d b = y[i]; x[i] = v2d{c * b.x, c * b.y}; }
    }
  }
}

// P += c Q with complex c   (linalg/assign_add_mul.c); element-wise, so P may be Q
__global__ __launch_bounds__(LA_BS) void caxpy_kernel(v2d *P, const v2d *Q, double cre, double cim, int ns, int N) {
  v2d *p = P + (size_t)blockIdx.y * ns;
  const v2d *q = Q + (size_t)blockIdx.y * ns;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) { const v2d a = p[i], b = q[i]; p[i] = v2d{a.x + cre * b.x - cim * b.y, a.y + cre * b.y + cim * b.x}; }
  }
}

// l = sigma_c * ( zc (.) k - beta * j ),  zc = z for spin 0,1 and conj(z) for spin 2,3,
// sigma_c = -1 on spin 2,3 when g5 is set.  Covers mul_one_pm_imu_inv, assign_mul_one_pm_imu[_inv],
// mul_one_pm_imu_sub_mul[_gamma5], gamma5.  Element-wise => alias-safe for l==k, l==j.
__global__ __launch_bounds__(LA_BS) void diag_kernel(v2d *L, const v2d *K, const v2d *J, double zre, double zim, int beta, int g5,
                                                     int ns, int N) {
  const int comp = blockIdx.y;
  const bool lower = comp >= 6;
  const double zi = lower ? -zim : zim;
  const double sg = (lower && g5) ? -1.0 : 1.0;
  v2d *l = L + (size_t)comp * ns;
  const v2d *k = K + (size_t)comp * ns;
  const v2d *j = J ? J + (size_t)comp * ns : nullptr;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      const v2d a = k[i];
      v2d r = v2d{zre * a.x - zi * a.y, zre * a.y + zi * a.x};
      if (beta) r -= j[i];
      l[i] = v2d{sg * r.x, sg * r.y};
    }
  }
}

// ---- complex products and updates, one field or a group of G fields against one (the chronological guess, chrono.hip)
// The per-thread accumulation, the sum over the block and the final pass are one piece of code for every G, and the four products of
// a term are rounded one by one: a value of a group carries the bits of the same product taken alone, and <S, S> has an imaginary
// part of exactly zero.  (This file is built with -ffp-contract=fast, which fuses across statements whatever a pragma says; a product
// that has passed through an empty asm statement is a value the compiler cannot fuse into the addition behind it.)
#define CSG_GROUP 8       // fields per launch of the update and combination kernels
#define CSG_DOT_GROUP 6   // ... of the product kernel: two accumulators per field, and seven fields no longer fit the 64 registers of eight waves per SIMD
template <int G> struct CsgFields { v2d *f[G]; double c[2 * G]; };

__device__ __forceinline__ void cdot_add(double &re, double &im, const v2d a, const v2d b) {   // += conj(a) b   (scalar_prod_body.c:52)
  double rr = a.x * b.x, ii = a.y * b.y, ri = a.x * b.y, ir = a.y * b.x;
  asm("" : "+v"(rr), "+v"(ii), "+v"(ri), "+v"(ir));
  re += rr + ii;
  im += ri - ir;
}

// out[2g], out[2g+1] = Re, Im <S_g, R>: block sums of value k at partials[k * 12 * gridDim.x + ...], the layout of block_reduce_store per value
template <int G>
__global__ __launch_bounds__(LA_BS, 8) void csg_dot_kernel(const CsgFields<G> S, const v2d *R, int ns, int N, double *partials) {
  __shared__ double wsum[2 * G][LA_BS / 64];
  const size_t off = (size_t)blockIdx.y * ns;
  const v2d *r = R + off;
  double re[G], im[G];
#pragma unroll
  for (int g = 0; g < G; g++) re[g] = im[g] = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      const v2d b = r[i];
#pragma unroll
      for (int g = 0; g < G; g++) cdot_add(re[g], im[g], S.f[g][off + i], b);
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int g = 0; g < G; g++) {
    const double a = tmhip_wave_sum(re[g]), b = tmhip_wave_sum(im[g]);
    if (lane == 0) { wsum[2 * g][w] = a; wsum[2 * g + 1][w] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * G) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LA_BS / 64; k++) s += wsum[threadIdx.x][k];
    partials[(size_t)threadIdx.x * 12 * gridDim.x + blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

// value k = blockIdx.x: the fixed-order pass of reduce_final_kernel over its n block sums
__global__ __launch_bounds__(256) void reduce_final_multi_kernel(const double *__restrict__ partials, int n, double *out) {
  __shared__ double sm[256];
  const double *p = partials + (size_t)blockIdx.x * n;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += p[i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

// R_g -= c_g S   (linalg/assign_diff_mul.c)
template <int G>
__global__ __launch_bounds__(LA_BS, 8) void csg_axpy_kernel(const CsgFields<G> R, const v2d *S, int ns, int N) {
  const size_t off = (size_t)blockIdx.y * ns;
  const v2d *s = S + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      const v2d b = s[i];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const double cre = R.c[2 * g], cim = R.c[2 * g + 1];
        const v2d a = R.f[g][off + i];
        R.f[g][off + i] = v2d{a.x - cre * b.x + cim * b.y, a.y - cre * b.y - cim * b.x};
      }
    }
  }
}

// P = [P +] c_{G-1} V_{G-1} + ... + c_0 V_0, added in that order   (linalg/mul.c, then linalg/assign_add_mul.c per field); element-wise: P may be a V_g
template <int G, bool ACC>
__global__ __launch_bounds__(LA_BS, 8) void csg_lincomb_kernel(v2d *P, const CsgFields<G> V, int ns, int N) {
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *p = P + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) {
      v2d acc = ACC ? p[i] : v2d{0.0, 0.0};
#pragma unroll
      for (int g = G - 1; g >= 0; g--) {
        const double cre = V.c[2 * g], cim = V.c[2 * g + 1];
        const v2d b = V.f[g][off + i];
        if (!ACC && g == G - 1) acc = v2d{cre * b.x - cim * b.y, cre * b.y + cim * b.x};
        else acc = v2d{acc.x + cre * b.x - cim * b.y, acc.y + cre * b.y + cim * b.x};
      }
      p[i] = acc;
    }
  }
}

// ---- the two streams of the correction monomials (rational.hip; monomial/ratcor_monomial.c:192-206,211-212, ndratcor_monomial.c:212-240)
// out = c (in + rmu_{np-1} chi_{np-1} + ... + rmu_0 chi_0) for one flavour or both (blockIdx.z): the accumulator stays in a register,
// `in` and every chi_j are read once, out is written once.  The additions are those of stream_kernel<0> in the reference's order
// (j downwards) and the factor is the product of stream_kernel<5>, so the result carries the bits of tmhip_assign, np calls of
// tmhip_assign_add_mul_r and (c != 1) tmhip_mul_r; c = 1 multiplies by one, which changes nothing.  One site per thread: the np
// loads of a thread are independent of its sum and the loop is unrolled by four to keep them in flight.  Element-wise: out may be in.
struct RatSumArgs {
  const v2d *in[2], *chi[2][TMHIP_RAT_SUM_MAX];
  v2d *out[2];
  double rmu[TMHIP_RAT_SUM_MAX], c;
  int np, ns, N;
};
__global__ __launch_bounds__(LA_BS, 8) void rat_sum_kernel(const RatSumArgs a) {
  const int i = blockIdx.x * LA_BS + threadIdx.x;
  if (i >= a.N) return;
  const int f = blockIdx.z;
  const size_t off = (size_t)blockIdx.y * a.ns + i;
  v2d acc = a.in[f][off];
#pragma unroll 4
  for (int j = a.np - 1; j >= 0; j--) {
    const double c = a.rmu[j];
    const v2d b = a.chi[f][j][off];
    acc = v2d{acc.x + c * b.x, acc.y + c * b.y};
  }
  a.out[f][off] = v2d{a.c * acc.x, a.c * acc.y};
}

// K_f = K_f - L_f and the block sums of |K_f|^2, flavour f = blockIdx.z: the subtraction of stream_kernel<2> and then, on the value just
// stored, the lines of sqnorm_kernel -- the same per-thread order, block sum and partials layout (flavour f at partials + f * 12 *
// gridDim.x), so that the final pass below returns the bits of tmhip_diff followed by tmhip_square_norm
struct DiffSqArgs { v2d *k[2]; const v2d *l[2]; };
__global__ __launch_bounds__(LA_BS) void diff_sqnorm_kernel(const DiffSqArgs a, int ns, int N, double *partials) {
  v2d *k = a.k[blockIdx.z] + (size_t)blockIdx.y * ns;
  const v2d *l = a.l[blockIdx.z] + (size_t)blockIdx.y * ns;
  double acc = 0.0;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int u = 0; u < LA_UNROLL; u++) {
    const int i = base + u * LA_BS;
    if (i < N) { const v2d d = k[i] - l[i]; k[i] = d; acc += d.x * d.x + d.y * d.y; }
  }
  block_reduce_store(acc, partials + (size_t)blockIdx.z * 12 * gridDim.x);
}


// ---- the two three-field complex singles of BiCGstab (solver/bicgstab_complex.c:98,111).  grid.y = the planes of the field: twelve of
// an EO field, twenty-four of a FULL one (its odd half follows its even half at the same stride), n sites per plane.  Element-wise: R may
// be S or U.  MODE 0: R += c1 S + c2 U   (linalg/assign_add_mul_add_mul.c:42-60)   1: R = c2 (R + c1 S) + U   (linalg/assign_mul_bra_add_mul_ket_add.c:44-63)
template <int MODE>
__global__ __launch_bounds__(LA_BS, 8) void cplx3_kernel(v2d *R, const v2d *S, const v2d *U, double c1re, double c1im, double c2re, double c2im,
                                                         int ns, int n) {
  const size_t off = (size_t)blockIdx.y * ns;
  v2d *r = R + off;
  const v2d *s = S + off, *u = U + off;
  const int base = blockIdx.x * LA_BS * LA_UNROLL + threadIdx.x;
#pragma unroll
  for (int k = 0; k < LA_UNROLL; k++) {
    const int i = base + k * LA_BS;
    if (i < n) {
      const v2d a = r[i], b = s[i], c = u[i];
      r[i] = MODE == 0 ? tmhip_add_mul_add_mul(a, c1re, c1im, b, c2re, c2im, c) : tmhip_mul_bra_add_mul_ket_add(a, c1re, c1im, b, c2re, c2im, c);
    }
  }
}

// fp64 fields of one kind and stride; N = VOLUME for FULL fields, 0 <= N <= VOLUME/2 for EO fields.  *planes, *n: the launch shape
static int check_cplx3(tmhip_ctx *ctx, const char *who, tmhip_field *R, tmhip_field *S, tmhip_field *U, int N, int *planes, int *n) {
  if (!R || !S || !U) TMHIP_FAIL("%s: null field", who);
  if (R->prec || S->prec || U->prec) TMHIP_FAIL("%s: fp64 fields only", who);
  if (S->kind != R->kind || U->kind != R->kind || S->ns != R->ns || U->ns != R->ns) TMHIP_FAIL("%s: the three fields must be of one kind", who);
  if (R->kind == TMHIP_FIELD_FULL) {
    if (N != ctx->V) TMHIP_FAIL("%s: N = %d, FULL fields take N = VOLUME = %d", who, N, ctx->V);
    *planes = 24; *n = ctx->Vh;
  } else {
    if (N < 0 || N > ctx->Vh) TMHIP_FAIL("%s: N = %d is outside [0, VOLUME/2 = %d]", who, N, ctx->Vh);
    *planes = 12; *n = N;
  }
  return 0;
}

static int check_eo(const tmhip_field *f, const char *who) {
  if (!f || f->kind != TMHIP_FIELD_EO || f->prec != 0) { fprintf(stderr, "[tmlqcd_hip] %s: needs a one-parity (EO) field\n", who); return 1; }
  return 0;
}

// MPI_Allreduce(..., MPI_SUM) of the reference (square_norm.c:314): one double over RCCL
int tmhip_rank_sum(tmhip_ctx *ctx) {
  if (ctx->direct.on && ctx->direct.sums_on) return tmhip_direct_allreduce(ctx, ctx->result_dev);
  if (ctx->shm) return tmhip_shm_allreduce(ctx, ctx->stream, ctx->result_dev, 1);
  TMHIP_NCCL_CHECK(ncclAllReduce(ctx->result_dev, ctx->result_dev, 1, ncclDouble, ncclSum, ctx->comm_red, ctx->stream));
  return 0;
}

int tmhip_reduce_finish(tmhip_ctx *ctx, int nblocks, int parallel, double *out) {
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->partials, nblocks, ctx->result_dev);
  if (parallel && tmhip_reduce_over_ranks(ctx) && tmhip_rank_sum(ctx)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(ctx->result_host, ctx->result_dev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = *ctx->result_host;
  return tmhip_check_async_error(ctx);
}

// ---- the complex singles and their batched forms: the host cuts n fields into groups of at most CSG_GROUP, one launch per group
static int csg_buffers(tmhip_ctx *ctx) {
  if (ctx->csg_partials) return 0;
  const size_t nb = (size_t)12 * la_grid(ctx->Vh).x;
  TMHIP_CHECK(hipMalloc((void **)&ctx->csg_partials, 2 * TMHIP_CSG_MAX * nb * sizeof(double)));
  TMHIP_CHECK(hipMalloc((void **)&ctx->csg_res_dev, 2 * TMHIP_CSG_MAX * sizeof(double)));
  TMHIP_CHECK(hipHostMalloc((void **)&ctx->csg_res_host, 2 * TMHIP_CSG_MAX * sizeof(double)));
  return 0;
}
static int csg_check(tmhip_ctx *ctx, int n, tmhip_field *const *f, tmhip_field *one, const char *who) {
  if (n < 1 || n > TMHIP_CSG_MAX) TMHIP_FAIL("%s: n = %d fields, must be in [1, %d]", who, n, TMHIP_CSG_MAX);
  if (!f || check_eo(one, who)) return 1;
  for (int i = 0; i < n; i++) if (check_eo(f[i], who) || f[i]->ns != one->ns) return 1;
  return 0;
}
template <int G> static CsgFields<G> csg_pack(tmhip_field *const *f, const double *c) {
  CsgFields<G> a;
  for (int g = 0; g < G; g++) { a.f[g] = f[g]->d; a.c[2 * g] = c ? c[2 * g] : 0.0; a.c[2 * g + 1] = c ? c[2 * g + 1] : 0.0; }
  return a;
}
// calls body(std::integral_constant<int, G>) for the run-time group size g in [1, CSG_GROUP]
template <int G, class F> static inline void csg_dispatch(int g, F body) {
  if (g == G) body(std::integral_constant<int, G>());
  else if constexpr (G > 1) csg_dispatch<G - 1>(g, body);
}

// block sums of <S_i, R>, i < n, into csg_partials and one final pass into csg_res_dev[0 .. 2n)
static int csg_dot_enqueue(tmhip_ctx *ctx, int n, tmhip_field *const *S, tmhip_field *R, int N) {
  if (csg_buffers(ctx)) return 1;
  const dim3 grid = la_grid(N);
  const size_t per = (size_t)grid.x * grid.y;
  for (int first = 0; first < n; first += CSG_DOT_GROUP) {
    const int g = n - first < CSG_DOT_GROUP ? n - first : CSG_DOT_GROUP;
    csg_dispatch<CSG_DOT_GROUP>(g, [&](auto Gc) {
      constexpr int G = decltype(Gc)::value;
      hipLaunchKernelGGL(csg_dot_kernel<G>, grid, dim3(LA_BS), 0, ctx->stream, csg_pack<G>(S + first, nullptr), (const v2d *)R->d, R->ns, N,
                         ctx->csg_partials + 2 * first * per);
    });
  }
  hipLaunchKernelGGL(reduce_final_multi_kernel, dim3(2 * n), dim3(256), 0, ctx->stream, (const double *)ctx->csg_partials, (int)per, ctx->csg_res_dev);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" {

int tmhip_square_norm(tmhip_ctx *ctx, tmhip_field *P, int N, int parallel, double *out) {
  if (check_eo(P, "square_norm")) return 1;
  LA_CHECK_N("square_norm", *out = 0.0);
  const dim3 g = la_grid(N);
  hipLaunchKernelGGL(sqnorm_kernel, g, dim3(LA_BS), 0, ctx->stream, P->d, P->ns, N, ctx->partials);
  return tmhip_reduce_finish(ctx, g.x * g.y, parallel, out);
}

int tmhip_scalar_prod_r(tmhip_ctx *ctx, tmhip_field *S, tmhip_field *R, int N, int parallel, double *out) {
  if (check_eo(S, "scalar_prod_r") || check_eo(R, "scalar_prod_r")) return 1;
  LA_CHECK_N("scalar_prod_r", *out = 0.0);
  const dim3 g = la_grid(N);
  hipLaunchKernelGGL(dotr_kernel, g, dim3(LA_BS), 0, ctx->stream, S->d, R->d, S->ns, N, ctx->partials);
  return tmhip_reduce_finish(ctx, g.x * g.y, parallel, out);
}

int tmhip_assign_mul_add_r_and_square(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N, int parallel,
                                      double *out) {
  if (check_eo(R, "assign_mul_add_r_and_square") || check_eo(S, "assign_mul_add_r_and_square")) return 1;
  LA_CHECK_N("assign_mul_add_r_and_square", *out = 0.0);
  const dim3 g = la_grid(N);
  hipLaunchKernelGGL(xpay_sq_kernel, g, dim3(LA_BS), 0, ctx->stream, R->d, c, S->d, R->ns, N, ctx->partials);
  return tmhip_reduce_finish(ctx, g.x * g.y, parallel, out);
}

int tmhip_assign_add_mul_r(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, double c, int N) {
  if (check_eo(P, "assign_add_mul_r") || check_eo(Q, "assign_add_mul_r")) return 1;
  LA_CHECK_N("assign_add_mul_r", (void)0);
  hipLaunchKernelGGL(stream_kernel<0>, la_grid(N), dim3(LA_BS), 0, ctx->stream, P->d, Q->d, (const v2d *)nullptr, c, P->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_assign_add_mul(tmhip_ctx *ctx, tmhip_field *P, tmhip_field *Q, double c_re, double c_im, int N) {
  if (check_eo(P, "assign_add_mul") || check_eo(Q, "assign_add_mul")) return 1;
  LA_CHECK_N("assign_add_mul", (void)0);
  hipLaunchKernelGGL(caxpy_kernel, la_grid(N), dim3(LA_BS), 0, ctx->stream, P->d, (const v2d *)Q->d, c_re, c_im, P->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_assign_mul_add_r(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N) {
  if (check_eo(R, "assign_mul_add_r") || check_eo(S, "assign_mul_add_r")) return 1;
  LA_CHECK_N("assign_mul_add_r", (void)0);
  hipLaunchKernelGGL(stream_kernel<1>, la_grid(N), dim3(LA_BS), 0, ctx->stream, R->d, S->d, (const v2d *)nullptr, c, R->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_diff(tmhip_ctx *ctx, tmhip_field *Q, tmhip_field *R, tmhip_field *S, int N) {
  if (check_eo(Q, "diff") || check_eo(R, "diff") || check_eo(S, "diff")) return 1;
  LA_CHECK_N("diff", (void)0);
  hipLaunchKernelGGL(stream_kernel<2>, la_grid(N), dim3(LA_BS), 0, ctx->stream, Q->d, R->d, S->d, 0.0, Q->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_add(tmhip_ctx *ctx, tmhip_field *Q, tmhip_field *R, tmhip_field *S, int N) {
  if (check_eo(Q, "add") || check_eo(R, "add") || check_eo(S, "add")) return 1;
  LA_CHECK_N("add", (void)0);
  hipLaunchKernelGGL(stream_kernel<4>, la_grid(N), dim3(LA_BS), 0, ctx->stream, Q->d, R->d, S->d, 0.0, Q->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_mul_r(tmhip_ctx *ctx, tmhip_field *R, double c, tmhip_field *S, int N) {
  if (check_eo(R, "mul_r") || check_eo(S, "mul_r")) return 1;
  LA_CHECK_N("mul_r", (void)0);
  hipLaunchKernelGGL(stream_kernel<5>, la_grid(N), dim3(LA_BS), 0, ctx->stream, R->d, S->d, (const v2d *)nullptr, c, R->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_assign(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, int N) {
  if (check_eo(R, "assign") || check_eo(S, "assign")) return 1;
  LA_CHECK_N("assign", (void)0);
  if (R->d == S->d) return 0;
  hipLaunchKernelGGL(stream_kernel<3>, la_grid(N), dim3(LA_BS), 0, ctx->stream, R->d, S->d, (const v2d *)nullptr, 0.0, R->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_rat_sum_nd(tmhip_ctx *ctx, tmhip_field *out_up, tmhip_field *out_dn, tmhip_field *in_up, tmhip_field *in_dn, tmhip_field *const *chi_up,
                     tmhip_field *const *chi_dn, const double *rmu, int np, double c) {
  const int nf = out_dn || in_dn || chi_dn ? 2 : 1;
  const char *who = nf == 2 ? "rat_sum_nd" : "rat_sum";
  if (np < 1 || np > TMHIP_RAT_SUM_MAX) TMHIP_FAIL("%s: np = %d is outside [1, %d]", who, np, TMHIP_RAT_SUM_MAX);
  if (!chi_up || !rmu || (nf == 2 && !chi_dn)) TMHIP_FAIL("%s: null argument", who);
  if (check_eo(out_up, who) || check_eo(in_up, who) || (nf == 2 && (check_eo(out_dn, who) || check_eo(in_dn, who)))) return 1;
  RatSumArgs a;
  memset(&a, 0, sizeof(a));
  a.in[0] = in_up->d; a.out[0] = out_up->d;
  if (nf == 2) { a.in[1] = in_dn->d; a.out[1] = out_dn->d; }
  for (int f = 0; f < nf; f++) {
    tmhip_field *const *chi = f ? chi_dn : chi_up;
    tmhip_field *o = f ? out_dn : out_up, *in = f ? in_dn : in_up;
    if (in->ns != out_up->ns || o->ns != out_up->ns) TMHIP_FAIL("%s: fields with different strides", who);
    for (int j = 0; j < np; j++) {
      if (check_eo(chi[j], who)) return 1;
      if (chi[j]->ns != out_up->ns) TMHIP_FAIL("%s: fields with different strides (chi[%d])", who, j);
      if (chi[j]->d == o->d) TMHIP_FAIL("%s: out is chi[%d] (only `in` may be the output)", who, j);
      a.chi[f][j] = chi[j]->d;
    }
  }
  if (nf == 2 && (out_up->d == out_dn->d || out_up->d == in_dn->d || out_dn->d == in_up->d)) TMHIP_FAIL("%s: the two flavours share a field", who);
  for (int j = 0; j < np; j++) a.rmu[j] = rmu[j];
  a.c = c; a.np = np; a.ns = out_up->ns; a.N = ctx->Vh;
  TMHIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(rat_sum_kernel, dim3((ctx->Vh + LA_BS - 1) / LA_BS, 12, nf), dim3(LA_BS), 0, ctx->stream, a);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_rat_sum(tmhip_ctx *ctx, tmhip_field *out, tmhip_field *in, tmhip_field *const *chi, const double *rmu, int np, double c) {
  return tmhip_rat_sum_nd(ctx, out, nullptr, in, nullptr, chi, nullptr, rmu, np, c);
}

int tmhip_diff_sqnorm_nd(tmhip_ctx *ctx, tmhip_field *k_up, tmhip_field *k_dn, tmhip_field *l_up, tmhip_field *l_dn, double *out) {
  const int nf = k_dn || l_dn ? 2 : 1;
  const char *who = nf == 2 ? "diff_sqnorm_nd" : "diff_sqnorm";
  if (!out) TMHIP_FAIL("%s: null argument", who);
  if (check_eo(k_up, who) || check_eo(l_up, who) || (nf == 2 && (check_eo(k_dn, who) || check_eo(l_dn, who)))) return 1;
  if (l_up->ns != k_up->ns || (nf == 2 && (k_dn->ns != k_up->ns || l_dn->ns != k_up->ns))) TMHIP_FAIL("%s: fields with different strides", who);
  if (nf == 2 && (k_up->d == k_dn->d || k_up->d == l_dn->d || k_dn->d == l_up->d)) TMHIP_FAIL("%s: the two flavours share a field", who);
  if (tmhip_reduce_over_ranks(ctx)) TMHIP_FAIL("%s: rank-local; on a rank that sums over ranks call tmhip_diff and tmhip_square_norm", who);
  TMHIP_CHECK(hipSetDevice(ctx->device));
  if (csg_buffers(ctx)) return 1;
  DiffSqArgs a;
  a.k[0] = k_up->d; a.l[0] = l_up->d;
  a.k[1] = nf == 2 ? k_dn->d : nullptr; a.l[1] = nf == 2 ? l_dn->d : nullptr;
  const dim3 g = la_grid(ctx->Vh);
  hipLaunchKernelGGL(diff_sqnorm_kernel, dim3(g.x, g.y, nf), dim3(LA_BS), 0, ctx->stream, a, k_up->ns, ctx->Vh, ctx->csg_partials);
  hipLaunchKernelGGL(reduce_final_multi_kernel, dim3(nf), dim3(256), 0, ctx->stream, (const double *)ctx->csg_partials, (int)(g.x * g.y), ctx->csg_res_dev);
  TMHIP_CHECK(hipGetLastError());
  TMHIP_CHECK(hipMemcpyAsync(ctx->csg_res_host, ctx->csg_res_dev, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = nf == 2 ? ctx->csg_res_host[0] + ctx->csg_res_host[1] : ctx->csg_res_host[0];   // square_norm(k_up) + square_norm(k_dn), ndratcor_monomial.c:240
  return tmhip_check_async_error(ctx);
}

int tmhip_diff_sqnorm(tmhip_ctx *ctx, tmhip_field *k, tmhip_field *l, double *out) { return tmhip_diff_sqnorm_nd(ctx, k, nullptr, l, nullptr, out); }

int tmhip_multi_scalar_prod(tmhip_ctx *ctx, int n, tmhip_field *const *S, tmhip_field *R, int N, double *out) {
  if (csg_check(ctx, n, S, R, "multi_scalar_prod")) return 1;
  if (tmhip_reduce_over_ranks(ctx)) TMHIP_FAIL("multi_scalar_prod: rank-local; on a rank that sums over ranks call tmhip_scalar_prod per field");
  LA_CHECK_N("multi_scalar_prod", memset(out, 0, 2 * n * sizeof(double)));
  if (csg_dot_enqueue(ctx, n, S, R, N)) return 1;
  TMHIP_CHECK(hipMemcpyAsync(ctx->csg_res_host, ctx->csg_res_dev, 2 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  memcpy(out, ctx->csg_res_host, 2 * n * sizeof(double));
  return tmhip_check_async_error(ctx);
}

int tmhip_scalar_prod(tmhip_ctx *ctx, tmhip_field *S, tmhip_field *R, int N, int parallel, double out[2]) {
  if (csg_check(ctx, 1, &S, R, "scalar_prod")) return 1;
  LA_CHECK_N("scalar_prod", out[0] = out[1] = 0.0);
  if (csg_dot_enqueue(ctx, 1, &S, R, N)) return 1;
  if (parallel && tmhip_reduce_over_ranks(ctx)) {
    for (int k = 0; k < 2; k++) {   // the one-value sum over the ranks, once per part
      TMHIP_CHECK(hipMemcpyAsync(ctx->result_dev, ctx->csg_res_dev + k, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if (tmhip_rank_sum(ctx)) return 1;
      TMHIP_CHECK(hipMemcpyAsync(ctx->csg_res_dev + k, ctx->result_dev, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  TMHIP_CHECK(hipMemcpyAsync(ctx->csg_res_host, ctx->csg_res_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  TMHIP_CHECK(hipStreamSynchronize(ctx->stream));
  out[0] = ctx->csg_res_host[0]; out[1] = ctx->csg_res_host[1];
  return tmhip_check_async_error(ctx);
}

int tmhip_multi_assign_diff_mul(tmhip_ctx *ctx, int n, tmhip_field *const *R, tmhip_field *S, const double *c, int N) {
  if (csg_check(ctx, n, R, S, "multi_assign_diff_mul")) return 1;
  LA_CHECK_N("multi_assign_diff_mul", (void)0);
  for (int first = 0; first < n; first += CSG_GROUP) {
    const int g = n - first < CSG_GROUP ? n - first : CSG_GROUP;
    csg_dispatch<CSG_GROUP>(g, [&](auto Gc) {
      constexpr int G = decltype(Gc)::value;
      hipLaunchKernelGGL(csg_axpy_kernel<G>, la_grid(N), dim3(LA_BS), 0, ctx->stream, csg_pack<G>(R + first, c + 2 * first), (const v2d *)S->d, S->ns, N);
    });
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_assign_diff_mul(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, double c_re, double c_im, int N) {
  const double c[2] = {c_re, c_im};
  return tmhip_multi_assign_diff_mul(ctx, 1, &R, S, c, N);
}

int tmhip_assign_add_mul_add_mul(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, double c1_re, double c1_im, double c2_re,
                                 double c2_im, int N) {
  int planes, n;
  if (check_cplx3(ctx, "assign_add_mul_add_mul", R, S, U, N, &planes, &n)) return 1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(cplx3_kernel<0>, dim3(la_grid(n).x, planes), dim3(LA_BS), 0, ctx->stream, R->d, (const v2d *)S->d, (const v2d *)U->d, c1_re, c1_im,
                     c2_re, c2_im, R->ns, n);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_assign_mul_bra_add_mul_ket_add(tmhip_ctx *ctx, tmhip_field *R, tmhip_field *S, tmhip_field *U, double c1_re, double c1_im, double c2_re,
                                         double c2_im, int N) {
  int planes, n;
  if (check_cplx3(ctx, "assign_mul_bra_add_mul_ket_add", R, S, U, N, &planes, &n)) return 1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(cplx3_kernel<1>, dim3(la_grid(n).x, planes), dim3(LA_BS), 0, ctx->stream, R->d, (const v2d *)S->d, (const v2d *)U->d, c1_re, c1_im,
                     c2_re, c2_im, R->ns, n);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_lincomb(tmhip_ctx *ctx, tmhip_field *P, int n, tmhip_field *const *V, const double *c, int N) {
  if (csg_check(ctx, n, V, P, "lincomb")) return 1;
  LA_CHECK_N("lincomb", (void)0);
  // the group of the highest indices starts the sum, the groups below it add to P
  for (int end = n; end > 0; end -= CSG_GROUP) {
    const int g = end < CSG_GROUP ? end : CSG_GROUP, first = end - g;
    csg_dispatch<CSG_GROUP>(g, [&](auto Gc) {
      constexpr int G = decltype(Gc)::value;
      if (end == n) hipLaunchKernelGGL((csg_lincomb_kernel<G, false>), la_grid(N), dim3(LA_BS), 0, ctx->stream, P->d, csg_pack<G>(V + first, c + 2 * first), P->ns, N);
      else hipLaunchKernelGGL((csg_lincomb_kernel<G, true>), la_grid(N), dim3(LA_BS), 0, ctx->stream, P->d, csg_pack<G>(V + first, c + 2 * first), P->ns, N);
    });
  }
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

int tmhip_mul(tmhip_ctx *ctx, tmhip_field *R, double c_re, double c_im, tmhip_field *S, int N) {
  const double c[2] = {c_re, c_im};
  return tmhip_lincomb(ctx, R, 1, &S, c, N);
}

static int launch_diag(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j, double zre, double zim, int beta,
                       int g5, int N) {
  if (check_eo(l, "diag") || check_eo(k, "diag") || (j && check_eo(j, "diag"))) return 1;
  LA_CHECK_N("site-diagonal operator", (void)0);
  hipLaunchKernelGGL(diag_kernel, la_grid(N), dim3(LA_BS), 0, ctx->stream, l->d, k->d, j ? j->d : (const v2d *)nullptr, zre,
                     zim, beta, g5, l->ns, N);
  TMHIP_CHECK(hipGetLastError());
  return 0;
}

/* mul_one_pm_imu_inv_body.c:1-41 : z = nrm (1 -+ i mu) for sign = +-1 */
int tmhip_mul_one_pm_imu_inv(tmhip_ctx *ctx, tmhip_field *l, double _sign, int N) {
  const double nrm = 1. / (1. + ctx->mu * ctx->mu), sign = _sign < 0. ? 1. : -1.;
  return launch_diag(ctx, l, l, nullptr, nrm, sign * nrm * ctx->mu, 0, 0, N);
}
/* mul_one_pm_imu_inv_body.c:43-80 */
int tmhip_assign_mul_one_pm_imu_inv(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, double _sign, int N) {
  const double nrm = 1. / (1. + ctx->mu * ctx->mu), sign = _sign < 0. ? 1. : -1.;
  return launch_diag(ctx, l, k, nullptr, nrm, sign * nrm * ctx->mu, 0, 0, N);
}
/* tm_operators.c:669-720 : z = 1 +- i mu */
int tmhip_assign_mul_one_pm_imu(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, double _sign, int N) {
  const double sign = _sign < 0. ? -1. : 1.;
  return launch_diag(ctx, l, k, nullptr, 1., sign * ctx->mu, 0, 0, N);
}
/* tm_operators.c:627-667 */
int tmhip_mul_one_pm_imu(tmhip_ctx *ctx, tmhip_field *l, double _sign) {
  const double sign = _sign < 0. ? -1. : 1.;
  return launch_diag(ctx, l, l, nullptr, 1., sign * ctx->mu, 0, 0, ctx->Vh);
}
/* mul_one_pm_imu_sub_mul_body.c:1-48 */
int tmhip_mul_one_pm_imu_sub_mul(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j, double _sign, int N) {
  const double sign = _sign < 0. ? -1. : 1.;
  return launch_diag(ctx, l, k, j, 1., sign * ctx->mu, 1, 0, N);
}
/* tm_operators.c:813-858 */
int tmhip_mul_one_pm_imu_sub_mul_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j, double _sign) {
  const double sign = _sign < 0. ? -1. : 1.;
  return launch_diag(ctx, l, k, j, 1., sign * ctx->mu, 1, 1, ctx->Vh);
}
/* tm_operators.c:781-810 : l = g5 (k - j) */
int tmhip_mul_one_sub_mul_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, tmhip_field *j) {
  return launch_diag(ctx, l, k, j, 1., 0., 1, 1, ctx->Vh);
}
/* gamma.c:77-98 */
int tmhip_gamma5(tmhip_ctx *ctx, tmhip_field *l, tmhip_field *k, int N) {
  return launch_diag(ctx, l, k, nullptr, 1., 0., 0, 1, N);
}

}  // extern "C"
