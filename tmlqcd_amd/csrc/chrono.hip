// Chronological solver guess (solver/chrono_guess.c of the reference): the starting vector of A x = phi is the Galerkin solution in
// the span of the last n normalised solutions.  Host code only: the field work is the complex linalg of linalg.hip, either its
// batched kernels (one pass over the shared operand per group of fields, one host synchronisation per batch of products) or,
// with option "csg_batch" 0 and on ranks that sum over ranks, the one-field calls in sequence.
#include "tmhip_internal.h"
#include <complex>

typedef std::complex<double> cplx;

// Solves M y = b for the n x n row-major M (leading dimension ld), y returned in b; M is overwritten with its factors.
// Row-wise factorisation with a unit lower factor, the order of operations of solver/lu_solve.c:39-173: row 0 stays where it is;
// before row i (i >= 1) is reduced, the row among i .. n-1 whose entry in column i -- as it stands, the rows below i are not reduced
// yet -- has the largest squared modulus is exchanged with it (a later row wins only when strictly larger), with its right-hand side.
// Then the entries left of the diagonal become the multipliers, each divided by its pivot as soon as it is complete, and the entries
// from the diagonal on lose the part the rows above explain.  Forward and backward substitution follow.
static void csg_lu_solve(int n, cplx *M, int ld, cplx *b) {
  cplx rhs[TMHIP_CSG_MAX], y[TMHIP_CSG_MAX];
  for (int i = 0; i < n; i++) rhs[i] = b[i];
  for (int i = 1; i < n; i++) {
    int best = i;
    double size = std::norm(M[i * ld + i]);
    for (int row = i + 1; row < n; row++) {
      const double s = std::norm(M[row * ld + i]);
      if (s > size) { size = s; best = row; }
    }
    if (best != i) {
      for (int j = 0; j < n; j++) std::swap(M[i * ld + j], M[best * ld + j]);
      std::swap(rhs[i], rhs[best]);
    }
    for (int j = 0; j < n; j++) {
      const int upto = j < i ? j : i;
      cplx sum = 0.0;
      for (int k = 0; k < upto; k++) sum += M[i * ld + k] * M[k * ld + j];
      M[i * ld + j] -= sum;
      if (j < i) M[i * ld + j] = M[i * ld + j] / M[j * ld + j];
    }
  }
  for (int i = 0; i < n; i++) {
    y[i] = rhs[i];
    for (int j = 0; j < i; j++) y[i] -= M[i * ld + j] * y[j];
  }
  for (int i = n - 1; i >= 0; i--) {
    cplx t = y[i];
    for (int j = i + 1; j < n; j++) t -= M[i * ld + j] * b[j];
    b[i] = t / M[i * ld + i];
  }
}

// <S_i, R> for i < n: one batched call, or n single calls with the cross-rank sum
static int csg_dots(tmhip_ctx *ctx, bool batched, int n, tmhip_field *const *S, tmhip_field *R, int N, cplx *out) {
  double buf[2 * TMHIP_CSG_MAX];
  if (batched) { if (tmhip_multi_scalar_prod(ctx, n, S, R, N, buf)) return 1; }
  else for (int i = 0; i < n; i++) if (tmhip_scalar_prod(ctx, S[i], R, N, 1, buf + 2 * i)) return 1;
  for (int i = 0; i < n; i++) out[i] = cplx(buf[2 * i], buf[2 * i + 1]);
  return 0;
}

extern "C" {

int tmhip_chrono_guess(tmhip_ctx *ctx, tmhip_field *trial, tmhip_field *phi, tmhip_field *const *v, int n, int op, int N,
                       double *G_out, double *b_out) {
  if (!trial || trial->kind != TMHIP_FIELD_EO || trial->prec != 0) TMHIP_FAIL("chrono_guess: needs one-parity (EO) fp64 fields");
  if (n > TMHIP_CSG_MAX) TMHIP_FAIL("chrono_guess: %d vectors, at most %d are supported", n, TMHIP_CSG_MAX);
  if (N < 0 || N > ctx->Vh) TMHIP_FAIL("chrono_guess: N = %d is outside [0, VOLUME/2 = %d]", N, ctx->Vh);
  if (n <= 0 || N == 0) return tmhip_field_zero(ctx, trial);   // no operator is applied: `op` is not looked at
  if (!phi || !v) TMHIP_FAIL("chrono_guess: null argument");
  if (tmhip_op_check(ctx, "chrono_guess", TMHIP_S_CG, op, trial->kind)) return 1;   // before step 1 rewrites the caller's older vectors
  const bool batched = ctx->opt_csg_batch && !tmhip_reduce_over_ranks(ctx) && N == ctx->Vh;
  tmhip_field *newest = v[n - 1];
  cplx s[TMHIP_CSG_MAX], G[TMHIP_CSG_MAX * TMHIP_CSG_MAX], b[TMHIP_CSG_MAX];
  double c[2 * TMHIP_CSG_MAX];

  // 1. the older vectors lose their component along the newest one: <newest, v_i> = conj <v_i, newest>, bit for bit
  if (n > 1) {
    if (batched) {
      if (csg_dots(ctx, true, n - 1, v, newest, N, s)) return 1;
      for (int i = 0; i < n - 1; i++) { c[2 * i] = s[i].real(); c[2 * i + 1] = -s[i].imag(); }
      if (tmhip_multi_assign_diff_mul(ctx, n - 1, v, newest, c, N)) return 1;
    } else {
      for (int i = n - 2; i >= 0; i--) {
        if (tmhip_scalar_prod(ctx, newest, v[i], N, 1, c)) return 1;
        if (tmhip_assign_diff_mul(ctx, v[i], newest, c[0], c[1], N)) return 1;
      }
    }
  }
  // 2. the projected operator, column by column (upper triangle computed, lower mirrored), and the projected right-hand side
  for (int j = 0; j < n; j++) {
    if (tmhip_apply_op(ctx, op, trial, v[j])) return 1;
    if (csg_dots(ctx, batched, j + 1, v, trial, N, s)) return 1;
    for (int i = 0; i <= j; i++) { G[i * n + j] = s[i]; if (i != j) G[j * n + i] = std::conj(s[i]); }
  }
  if (csg_dots(ctx, batched, n, v, phi, N, b)) return 1;
  if (G_out) for (int i = 0; i < n * n; i++) { G_out[2 * i] = G[i].real(); G_out[2 * i + 1] = G[i].imag(); }
  if (b_out) for (int i = 0; i < n; i++) { b_out[2 * i] = b[i].real(); b_out[2 * i + 1] = b[i].imag(); }
  // 3. the small system, 4. the combination, newest vector first
  csg_lu_solve(n, G, n, b);
  for (int i = 0; i < n; i++) { c[2 * i] = b[i].real(); c[2 * i + 1] = b[i].imag(); }
  if (batched) return tmhip_lincomb(ctx, trial, n, v, c, N);
  if (tmhip_mul(ctx, trial, c[2 * (n - 1)], c[2 * (n - 1) + 1], newest, N)) return 1;
  for (int i = n - 2; i >= 0; i--) if (tmhip_assign_add_mul(ctx, trial, v[i], c[2 * i], c[2 * i + 1], N)) return 1;
  return 0;
}

int tmhip_csg_solve(int n, double *G, double *b) {
  if (n < 1 || n > TMHIP_CSG_MAX || !G || !b) TMHIP_FAIL("csg_solve: n = %d, must be in [1, %d]", n, TMHIP_CSG_MAX);
  static_assert(sizeof(cplx) == 2 * sizeof(double), "std::complex<double> is a (re, im) pair");
  csg_lu_solve(n, reinterpret_cast<cplx *>(G), n, reinterpret_cast<cplx *>(b));
  return 0;
}

int tmhip_chrono_add_solution(tmhip_ctx *ctx, tmhip_field *slot, tmhip_field *trial, int N) {
  double nrm;
  if (tmhip_square_norm(ctx, trial, N, 1, &nrm)) return 1;
  return tmhip_mul_r(ctx, slot, 1 / sqrt(nrm), trial, N);
}

}  // extern "C"
