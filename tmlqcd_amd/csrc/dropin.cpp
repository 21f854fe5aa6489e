// libtmlqcd_dropin.so -- tmLQCD's own hot-path symbols on top of the HIP core library.
//
// Host side only (no device code here): reads the reference's globals at call time and forwards to include/tmlqcd_hip.h.  Host arrays
// reach the device through in() / out() / done() of residency.cpp (dropin_internal.h), which keeps the registry host-pointer -> device
// mirror.  Each entry point cites the reference function it replaces (paths under /root/reference).
#include "dropin_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
// ---- globals owned by the host program (global.h, boundary.h) ----
extern int T, LX, LY, LZ, VOLUME, RAND, VOLUMEPLUSRAND;         /* global.h:82-84 */
extern int g_nproc_t, g_nproc_x, g_nproc_y, g_nproc_z;           /* global.h:206 */
extern int g_proc_coords[4];                                      /* global.h:207 */
extern su3 **g_gauge_field;                                       /* global.h:176 */
extern int g_update_gauge_copy;                                   /* global.h:73  */
extern int g_update_gauge_copy_32 __attribute__((weak));          /* global.h:74: the host's fp32 gauge copy is refreshed by host code when it needs it */
extern double g_mu;                                               /* global.h:198 */
extern double g_mu3 __attribute__((weak));                        /* global.h:197: odd-odd twist of the e/o clover operators is g_mu + g_mu3 */
extern TM_COMPLEX ka0, ka1, ka2, ka3;                             /* boundary.h:25 */
extern su3 ***sw __attribute__((weak));                           /* clovertm_operators.c:58 */
extern su3 ***sw_inv __attribute__((weak));                       /* clovertm_operators.c:59 */
extern double g_c_sw __attribute__((weak));                       /* global.h:198; a host program without it has no clover term */
extern double g_mubar __attribute__((weak));                       /* global.h:202: the doublet's twist ... */
extern double g_epsbar __attribute__((weak));                      /* ... and its flavour splitting */
extern double phmc_invmaxev __attribute__((weak));                 /* phmc.h:31 */
extern double phmc_cheb_evmin __attribute__((weak));               /* phmc.h:29: the interval of the Chebyshev sums (Ptilde_ndpsi) */
extern double phmc_cheb_evmax __attribute__((weak));
extern int phmc_exact_poly __attribute__((weak));                  /* phmc.c: 1 selects the branches of ndpoly_monomial.c that are not built */
extern int even_odd_flag __attribute__((weak));                    /* read_input.h: tmlqcd_hip_eigenvalues picks Qtm_pm_psi (set, the default) or Q_pm_psi */
extern double mixcg_innereps __attribute__((weak));               /* read_input.h:112 (only needed by mixed_cg_her) */
extern int mixcg_maxinnersolverit __attribute__((weak));          /* read_input.h:113 */
extern int g_sloppy_precision __attribute__((weak));              /* global.h:95 */
// Present in a full tmLQCD link (update_backward_gauge.c, libhmc.a); refreshes the HOST gauge
// copy that deriv_Sb.c:405-408,472 still reads, and clears g_update_gauge_copy.
void update_backward_gauge(su3 **const gf) __attribute__((weak));
// ILDG I/O (io/gauge_read.c, io/gauge_write.c): the reader's precision switch and the IO-check switch are owned by the input parser
extern int gauge_precision_read_flag __attribute__((weak));       /* read_input.l; default 64 */
extern int g_disable_IO_checks __attribute__((weak));             /* global.h:74 */
extern int g_disable_src_IO_checks __attribute__((weak));         /* global.h:74; read_spinor; default 0 */
extern int g_debug_level __attribute__((weak));                   /* global.h:70; read_spinor's prints; default 1 (default_input_values.h:115) */
extern int g_cart_id __attribute__((weak));                       /* global.h:206; default 0 */
extern int T_global __attribute__((weak));                        /* global.h:82 */
extern int L __attribute__((weak));                               /* global.h:82 */
// Q_pm_psi_prec: the preconditioner and its globals
extern void *g_precWS __attribute__((weak));                       /* global.h:267 */
extern double g_prec_sequence_d_dagger_d[3] __attribute__((weak)); /* solver/dirac_operator_eigenvectors.h:67 */
void spinorPrecondition(spinor *spinor_out, const spinor *spinor_in, void *ws, int tt, int ll, const TM_COMPLEX alpha,
                        unsigned int dagger, unsigned int autofft) __attribute__((weak));
// the two bispinor operators eigenvalues_bi is called with: the reference's functions, known here by their addresses only, never called
void Qtm_pm_ndbipsi(bispinor *const bisp_l, bispinor *const bisp_k) __attribute__((weak));   /* operator/tm_operators_nd.h */
void Qsw_pm_ndbipsi(bispinor *const bisp_l, bispinor *const bisp_k) __attribute__((weak));
extern paramsGaugeInfo GaugeInfo;   /* defined with read_gauge_field below */
}

namespace {

// ------------------------------------------------------------------ the session: one context and what it currently holds
struct Session {
  tmhip_ctx *c = nullptr;
  int device = -1;
  int dims[6] = {0, 0, 0, 0, 0, 0};
  unsigned long calls = 0;         // entry-point calls served (tmlqcd_hip_calls): lets an integration test see that a symbol resolved to this library
  bool gauge_uploaded = false;     // the current context holds a gauge copy
  bool dev_links_newer = false;    // resident mode: the device links are ahead of g_gauge_field until tmlqcd_hip_sync_gauge_to_host
  bool momenta_resident = false;   // the momenta live on the device (tmlqcd_hip_update_momenta), not re-uploaded by tmlqcd_hip_update_gauge
  bool clover_uploaded = false;
  bool sw_on_device = false;       // the device's 1+T belongs to the current links (tmlqcd_hip_sw_term, or the host's sw uploaded)
  bool deriv_pending = false;      // a force is accumulating in the device's derivative, not yet in hf->derivative
  bool deriv_made = false;         // some force has run on the device: its derivative accumulator exists
  tmhip_field *full_tmp = nullptr; // FULL-lattice scratch of Q_pm_psi / D_dagg_psi (tm_operators.c:380-397)
  tmhip_field *f32[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // device fields of the fp32 host-pointer symbols (Hopping_Matrix_32 ...)

  tmhip_ctx *context() {
    if (!c) {
      if (g_nproc_x != 1 || g_nproc_y != 1 || g_nproc_z != 1)
        die("only T-direction decomposition is supported (g_nproc_x/y/z must be 1)");
      if (device < 0) {
        const char *e = getenv("TMLQCD_HIP_DEVICE");
        device = e ? atoi(e) : 0;
      }
      residency_from_env();
      tmhip_geom g = {T, LX, LY, LZ, g_nproc_t < 1 ? 1 : g_nproc_t, g_proc_coords[0]};
      CK(tmhip_create(&g, device, &c));
      dims[0] = T; dims[1] = LX; dims[2] = LY; dims[3] = LZ; dims[4] = g.nproc_t; dims[5] = g.proc_t;
    } else if (dims[0] != T || dims[1] != LX || dims[2] != LY || dims[3] != LZ) {
      die("lattice extents changed after the first call");
    }
    return c;
  }
  // Re-read everything the reference reads through globals (SURVEY §8b "Data it reads through globals").
  tmhip_ctx *refresh(bool need_gauge) {
    context();
    calls++;
    const double ka[8] = {__real__ ka0, __imag__ ka0, __real__ ka1, __imag__ ka1,
                          __real__ ka2, __imag__ ka2, __real__ ka3, __imag__ ka3};
    CK(tmhip_set_ka(c, ka));
    CK(tmhip_set_mu(c, g_mu));
    CK(tmhip_set_mu3(c, &g_mu3 ? g_mu3 : 0.));
    if (need_gauge && (g_update_gauge_copy || !gauge_uploaded)) {   /* Hopping_Matrix.c:135-139 */
      // A raised flag always means "the host's links changed since the device last saw them": the device paths that bring both sides
      // to the same state (tmlqcd_hip_update_gauge, read_gauge_field, tmlqcd_hip_sync_gauge_to_host) clear it themselves
      // (links_in_step), so a raise that follows -- the reject step restoring the old links (update_tm.c), a host-side
      // reunitarisation -- is never mistaken for our own.
      if (update_backward_gauge) update_backward_gauge(g_gauge_field);  // host copy + flag, as the reference
      else g_update_gauge_copy = 0;
      CK(tmhip_set_gauge(c, &g_gauge_field[0][0]));
      dev_links_newer = false;                                          // the host's links are the truth again
      gauge_uploaded = true;
    }
    return c;
  }
  void ensure_clover() {
    if (!clover_uploaded) {
      if (!&sw || !&sw_inv || !sw || !sw_inv) die("clover operator called but the host program has no sw / sw_inv (init_sw_fields)");
      CK(tmhip_set_clover(c, &sw[0][0][0], &sw_inv[0][0][0]));
      clover_uploaded = true;
      sw_on_device = true;
    }
  }
  tmhip_ctx *refresh_clover() {
    refresh(true);
    ensure_clover();
    return c;
  }
  // a solve on row `op` of the operator table (op_table.h): a clover row needs the host's sw / sw_inv on the device
  tmhip_ctx *refresh_for(int op) { return tmhip_op_row_of(op)->clover ? refresh_clover() : refresh(true); }
  tmhip_ctx *refresh_unsplit(const char *who, const char *what) {
    if (g_nproc_t > 1) {
      char m[160];
      snprintf(m, sizeof(m), "%s: %s run on unsplit lattices only", who, what);
      die(m);
    }
    return refresh(true);
  }
  tmhip_ctx *refresh_nd(const char *who) {
    refresh_unsplit(who, "the doublet operators and solvers");
    CK(tmhip_set_nd(c, &g_mubar ? g_mubar : 0., &g_epsbar ? g_epsbar : 0., &phmc_invmaxev ? phmc_invmaxev : 1.));
    return c;
  }
  tmhip_ctx *refresh_rat(const char *who) { return refresh_unsplit(who, "the rational monomials"); }
  void clover_stale() { clover_uploaded = false; sw_on_device = false; }   // the links changed: 1+T and its inverse are not theirs any more
} ses;

// ------------------------------------------------------------------ the shapes the entry points come in
using Ctx = tmhip_ctx *;     // (short names for the parameter lists of the lambdas below)
using Fld = tmhip_field *;
// l = core(k) or core(k, j) on fields of one kind; which refresh made `c` is all that tells a plain operator from a clover one
template <class F> inline void apply(tmhip_ctx *c, int kind, spinor *l, const spinor *k, const spinor *j, F core) {
  tmhip_field *fk = in(c, k, kind), *fj = j ? in(c, j, kind) : nullptr, *fl = out(c, l, kind);
  core(c, fl, fk, fj);
  done(c, l);
}
#define EO_OP(NAME, REFRESH, CORE)                                                                                 \
  void NAME(spinor *const l, spinor *const k) {                                                                    \
    apply(REFRESH, TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { CK(CORE(c, fl, fk)); });       \
  }
// (l0, l1) = core(k0, k1) on one-parity fields: the doublet operators and the even/odd pairs of the full-lattice ones
template <class F> inline void apply2(tmhip_ctx *c, spinor *l0, spinor *l1, const spinor *k0, const spinor *k1, F core) {
  tmhip_field *fk0 = in(c, k0, TMHIP_FIELD_EO), *fk1 = in(c, k1, TMHIP_FIELD_EO);
  tmhip_field *fl0 = out(c, l0, TMHIP_FIELD_EO), *fl1 = out(c, l1, TMHIP_FIELD_EO);
  core(c, fl0, fl1, fk0, fk1);
  done(c, l0); done(c, l1);
}
#define ND_OP(NAME, CORE)                                                                                                              \
  void NAME(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c) {                                              \
    apply2(ses.refresh_nd(#NAME), l_s, l_c, k_s, k_c, [&](Ctx c, Fld fls, Fld flc, Fld fks, Fld fkc) { CK(CORE(c, fls, flc, fks, fkc)); }); \
  }

// The length-N element-wise routines (linalg, site-diagonal twists).  Up to three operands in the order they are handed to the
// registry: rd() is read, wr() is written, rw() is updated in place.  core(c, f0, f1, f2, n) runs once per part.
int kind_of_N(int N) {
  if (N == VOLUME / 2) return TMHIP_FIELD_EO;
  if (N == VOLUME) return TMHIP_FIELD_FULL;
  if (N > 0 && N < VOLUME) return KIND_LIN;
  die("linalg/site-diagonal call with N outside [0, VOLUME]");
}
tmhip_field *half(tmhip_field *f, int kind, int par) {
  if (kind == TMHIP_FIELD_EO) return f;
  return par ? tmhip_field_odd(f) : tmhip_field_even(f);
}
struct Opnd { const spinor *host; bool read, written; };
inline Opnd rd(const spinor *h) { return {h, true, false}; }
inline Opnd wr(const spinor *h) { return {h, false, true}; }
inline Opnd rw(const spinor *h) { return {h, true, true}; }
inline Opnd none() { return {nullptr, false, false}; }
template <class F> inline void lin_op(const int N, Opnd a0, Opnd a1, Opnd a2, F core) {
  tmhip_ctx *c = ses.refresh(false);
  if (N == 0) return;   /* an empty loop in the reference */
  const int kind = kind_of_N(N);
  const Parts pt = parts_of(kind, N);
  const Opnd a[3] = {a0, a1, a2};
  tmhip_field *f[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; i++) if (a[i].host) f[i] = a[i].read ? in(c, a[i].host, kind, N) : out(c, a[i].host, kind, N);
  for (int p = 0; p < pt.n; p++) core(c, f[0] ? half(f[0], kind, p) : nullptr, f[1] ? half(f[1], kind, p) : nullptr, f[2] ? half(f[2], kind, p) : nullptr, pt.cnt[p]);
  for (int i = 0; i < 3; i++) if (a[i].host && a[i].written) done(c, a[i].host);
}

// a stretch of device calls under another twist than g_mu (refresh() has set g_mu, and it is set again afterwards)
template <class F> inline void with_mu(tmhip_ctx *c, const double mu, F body) {
  CK(tmhip_set_mu(c, mu));
  body();
  CK(tmhip_set_mu(c, g_mu));
}

/* D_psi_body.c:314-316: with g_c_sw > 0 the site term of D_psi is the clover one, (1 + T(x) + i mu g5) from the host's sw array.
 * On the two parities of a full field that is Msw_full (clovertm_operators.c:96-110): new = (1 + T + i mu g5) own - H other. */
void d_psi_core(tmhip_ctx *c, tmhip_field *fp, tmhip_field *fq) {
  if (&g_c_sw && g_c_sw > 0.) {
    ses.ensure_clover();
    CK(tmhip_Msw_full(c, tmhip_field_even(fp), tmhip_field_odd(fp), tmhip_field_even(fq), tmhip_field_odd(fq)));
  } else {
    CK(tmhip_D_psi(c, fp, fq));
  }
}
tmhip_field *full_tmp(tmhip_ctx *c) {
  if (!ses.full_tmp) CK(tmhip_field_alloc(c, TMHIP_FIELD_FULL, &ses.full_tmp));
  return ses.full_tmp;
}
void g5_full(tmhip_ctx *c, tmhip_field *l, tmhip_field *k) {
  CK(tmhip_gamma5(c, tmhip_field_even(l), tmhip_field_even(k), VOLUME / 2));
  CK(tmhip_gamma5(c, tmhip_field_odd(l), tmhip_field_odd(k), VOLUME / 2));
}
/* tm_operators.c:380-388, 453-461: l = g5 D(+mu) g5 D(first_mu) k on the full lattice */
void q_pm_full(spinor *l, spinor *k, const double first_mu) {
  apply(ses.refresh(true), TMHIP_FIELD_FULL, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    tmhip_field *tmp = full_tmp(c);
    with_mu(c, first_mu, [&] { d_psi_core(c, fl, fk); g5_full(c, tmp, fl); });
    d_psi_core(c, fl, tmp);
    g5_full(c, fl, fl);
  });
}

// A force accumulates on the device: the first contribution since the last flush / tmlqcd_hip_update_momenta starts from zero; after
// each one hf->derivative receives the sum unless the mode is resident (lazy mode watches spinor arrays only).
void force_begin(tmhip_ctx *c) { if (!ses.deriv_pending) CK(tmhip_derivative_zero(c)); ses.deriv_made = true; }
void force_end(hamiltonian_field_t *const hf) {
  ses.deriv_pending = true;
  if (!resident()) tmlqcd_hip_flush_derivative(hf);
}

// ndrat and ndcloverrat: the same heatbath and acceptance bodies around their own core function
template <class Core> inline int nd_heatbath(const char *who, Core core, spinor *const pf, spinor *const pf2, const double *nu, const double *rnu, const int np,
                                             const double EVMaxInv, const int max_iter, const double eps_sq, const int rel_prec, double *energy0) {
  tmhip_ctx *c = ses.refresh_nd(who);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  int iters = -1;
  CK(core(c, fu, fd, nu, rnu, np, EVMaxInv, max_iter, eps_sq, rel_prec, energy0, &iters));
  done(c, pf); done(c, pf2);
  return iters;
}
template <class Core> inline int nd_acc(const char *who, Core core, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np,
                                        const int max_iter, const double eps_sq, const int rel_prec, double *energy1) {
  tmhip_ctx *c = ses.refresh_nd(who);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  int iters = -1;
  CK(core(c, fu, fd, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, &iters));
  return iters;
}

// fp32 twins on host spinor32 arrays: a small pool of device fields, see "fp32 twins" below
tmhip_field *f32(tmhip_ctx *c, int k) {
  if (!ses.f32[k]) CK(tmhip_field_alloc32(c, &ses.f32[k]));
  return ses.f32[k];
}
tmhip_field *in32(tmhip_ctx *c, int k, const spinor32 *host, int N) {
  tmhip_field *f = f32(c, k);
  CK(tmhip_field_upload32(c, f, host, N));
  return f;
}
void need_N32(int N, const char *who) {
  if (N < 0 || N > VOLUME / 2) { fprintf(stderr, "[tmlqcd_dropin] %s: N = %d outside [0, VOLUME/2] (fp32 fields are one-parity fields)\n", who, N); exit(1); }
}
template <class F> inline void team_once(F body) {
#pragma omp barrier
#pragma omp master
  body();
#pragma omp barrier
}

int chrono_guess_generic(spinor *const trial, spinor *const phi, spinor **const v, const int *index_array, const int n, const int V, matrix_mult f);
// The one lookup from the reference's functions to the rows of the operator table (op_table.h): the id `solver` (TMHIP_S_*) runs
// device-resident for f on N sites, or -1 -- f is no row, N is not the site count of the row's fields, or the solver does not take
// the row.  The FULL rows are not ours when g_c_sw > 0: there D_psi is Msw_full (d_psi_core), and Q_pm_psi is built on it.
int dev_op_of(matrix_mult f, const int N, const int solver) {
  static const struct { matrix_mult f; int id; } fn[] = {
#define X(ID, NAME, KIND, SW, FP32, SOLVERS) {&NAME, TMHIP_OP_##ID},
    TMHIP_OP_TABLE(X)
#undef X
  };
  for (const auto &e : fn) {
    if (e.f != f) continue;
    const tmhip_op_row *r = tmhip_op_row_of(e.id);
    const bool full = r->kind == TMHIP_FIELD_FULL;
    if (N != (full ? VOLUME : VOLUME / 2) || !tmhip_op_taken(r, solver) || (full && &g_c_sw && g_c_sw > 0.)) return -1;
    return e.id;
  }
  return -1;
}
// the same for the doublet (TMHIP_ND_OP_*)
int dev_nd_op_of(matrix_mult_nd f, const int N) {
  static const struct { matrix_mult_nd f; int id; } fn[] = {
#define X(ID, NAME, KIND, SW, FP32, SOLVERS) {&NAME, TMHIP_ND_OP_##ID},
    TMHIP_ND_OP_TABLE(X)
#undef X
  };
  for (const auto &e : fn) if (e.f == f) return N == VOLUME / 2 ? e.id : -1;
  return -1;
}
int op_kind(int op) { return tmhip_op_row_of(op)->kind; }   // the kind of the fields row `op` acts on
int cg_her_generic(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N, matrix_mult f);
int bicgstab_complex_generic(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N, matrix_mult f);
int cg_mms_tm_generic(spinor **const P, spinor *const Q, tmlqcd_solver_params *sp, double *cgmms_reached_prec);

}  // namespace

tmhip_ctx *ctx() { return ses.context(); }
tmhip_ctx *live_ctx() { return ses.c; }

extern "C" {

// ------------------------------------------------------------------ session control (the residency entry points: residency.cpp)
void tmlqcd_hip_set_device(int device) { ses.device = device; }
void tmlqcd_hip_comm_init(const char unique_id[128]) { CK(tmhip_comm_init(ctx(), unique_id)); }
void tmlqcd_hip_comm_init_shm(const char *job) { CK(tmhip_comm_init_shm(ctx(), job)); }
int tmlqcd_hip_comm_init_ipc(void) { return tmhip_comm_init_ipc(ctx()); }   // (non-zero: the faces stay on the communicator, on every rank -- not fatal)
unsigned long tmlqcd_hip_calls(void) { return ses.calls; }
void tmlqcd_hip_finalize(void) {
  if (!ses.c) return;
  release_all_mirrors(ses.c);
  if (ses.full_tmp) { tmhip_field_free(ses.c, ses.full_tmp); ses.full_tmp = nullptr; }
  for (int k = 0; k < 6; k++) if (ses.f32[k]) { tmhip_field_free(ses.c, ses.f32[k]); ses.f32[k] = nullptr; }
  tmhip_destroy(ses.c);
  ses.c = nullptr;
  ses.gauge_uploaded = false;
  ses.clover_stale();
  ses.dev_links_newer = ses.momenta_resident = false;
  ses.deriv_pending = ses.deriv_made = false;
}

// ------------------------------------------------------------------ stencil
/* operator/Hopping_Matrix.c:131-156 */
void Hopping_Matrix(const int ieo, spinor *const l, spinor *const k) {
  apply(ses.refresh(true), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { CK(tmhip_hopping_matrix(c, ieo, fl, fk)); });
}
/* operator/Hopping_Matrix_nocom.c:48-56 */
void Hopping_Matrix_nocom(const int ieo, spinor *const l, spinor *const k) {
  apply(ses.refresh(true), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { CK(tmhip_hopping_matrix_nocom(c, ieo, fl, fk)); });
}
/* operator/tm_times_Hopping_Matrix.c:72-153 */
void tm_times_Hopping_Matrix(const int ieo, spinor *const l, spinor *const k, TM_COMPLEX const cfactor) {
  apply(ses.refresh(true), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    CK(tmhip_tm_times_hopping_matrix(c, ieo, fl, fk, __real__ cfactor, __imag__ cfactor));
  });
}
/* operator/tm_sub_Hopping_Matrix.c:73-157 */
void tm_sub_Hopping_Matrix(const int ieo, spinor *const l, spinor *p, spinor *const k, TM_COMPLEX const cfactor) {
  apply(ses.refresh(true), TMHIP_FIELD_EO, l, k, p, [&](Ctx c, Fld fl, Fld fk, Fld fp) {
    CK(tmhip_tm_sub_hopping_matrix(c, ieo, fl, fp, fk, __real__ cfactor, __imag__ cfactor));
  });
}
/* operator/D_psi.c:1133-1140 -> D_psi_body.c:266-375 */
void D_psi(spinor *const P, spinor *const Q) {
  if (P == Q) {   /* D_psi_body.c:267-272 */
    printf("Error in D_psi (operator.c):\nArguments must be different spinor fields\nProgram aborted\n");
    exit(1);
  }
  apply(ses.refresh(true), TMHIP_FIELD_FULL, P, Q, nullptr, [&](Ctx c, Fld fp, Fld fq, Fld) { d_psi_core(c, fp, fq); });
}

// ------------------------------------------------------------------ e/o operators (tm_operators.c)
EO_OP(Qtm_plus_psi, ses.refresh(true), tmhip_Qtm_plus_psi)        /* tm_operators.c:172-177 */
EO_OP(Qtm_minus_psi, ses.refresh(true), tmhip_Qtm_minus_psi)      /* tm_operators.c:216-221 */
EO_OP(Mtm_plus_psi, ses.refresh(true), tmhip_Mtm_plus_psi)        /* tm_operators.c:245-250 */
EO_OP(Mtm_minus_psi, ses.refresh(true), tmhip_Mtm_minus_psi)      /* tm_operators.c:289-294 */
EO_OP(Qtm_pm_psi, ses.refresh(true), tmhip_Qtm_pm_psi)            /* tm_operators.c:338-345 */
EO_OP(Qtm_plus_sym_psi, ses.refresh(true), tmhip_Qtm_plus_sym_psi)            /* tm_operators.c:186-192 */
EO_OP(Qtm_minus_sym_psi, ses.refresh(true), tmhip_Qtm_minus_sym_psi)          /* tm_operators.c:223-229 */
EO_OP(Mtm_plus_sym_psi, ses.refresh(true), tmhip_Mtm_plus_sym_psi)            /* tm_operators.c:259-265 */
EO_OP(Mtm_minus_sym_psi, ses.refresh(true), tmhip_Mtm_minus_sym_psi)          /* tm_operators.c:296-302 */
EO_OP(Mtm_plus_sym_dagg_psi, ses.refresh(true), tmhip_Mtm_plus_sym_dagg_psi)  /* tm_operators.c:312-322 */
EO_OP(Qtm_pm_sym_psi, ses.refresh(true), tmhip_Qtm_pm_sym_psi)                /* tm_operators.c:347-364 */
void Qtm_plus_sym_psi_nocom(spinor *const l, spinor *const k) { Qtm_plus_sym_psi(l, k); }   /* :194-200 */
void Mtm_plus_sym_psi_nocom(spinor *const l, spinor *const k) { Mtm_plus_sym_psi(l, k); }   /* :267-273 */
void Mtm_minus_sym_psi_nocom(spinor *const l, spinor *const k) { Mtm_minus_sym_psi(l, k); } /* :304-310 */
/* The _nocom variants differ from the above only by skipping the halo exchange
 * (tm_operators.c:179-184,252-257,369-379); on one GPU they are the same function. */
void Qtm_plus_psi_nocom(spinor *const l, spinor *const k) { Qtm_plus_psi(l, k); }
void Mtm_plus_psi_nocom(spinor *const l, spinor *const k) { Mtm_plus_psi(l, k); }
void Qtm_pm_psi_nocom(spinor *const l, spinor *const k) { Qtm_pm_psi(l, k); }
/* tm_operators.c:508-526 */
void H_eo_tm_inv_psi(spinor *const l, spinor *const k, const int ieo, const double sign) {
  apply(ses.refresh(true), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { CK(tmhip_H_eo_tm_inv_psi(c, fl, fk, ieo, sign)); });
}
/* tm_operators.c:117-128 */
void M_full(spinor *const En, spinor *const On, spinor *const E, spinor *const O) {
  apply2(ses.refresh(true), En, On, E, O, [&](Ctx c, Fld fen, Fld fon, Fld fe, Fld fo) { CK(tmhip_M_full(c, fen, fon, fe, fo)); });
}
/* tm_operators.c:130-143 */
void Q_full(spinor *const En, spinor *const On, spinor *const E, spinor *const O) {
  apply2(ses.refresh(true), En, On, E, O, [&](Ctx c, Fld fen, Fld fon, Fld fe, Fld fo) {
    CK(tmhip_M_full(c, fen, fon, fe, fo));
    CK(tmhip_gamma5(c, fen, fen, VOLUME / 2));
    CK(tmhip_gamma5(c, fon, fon, VOLUME / 2));
  });
}
/* tm_operators.c:145-155 */
void M_minus_1_timesC(spinor *const En, spinor *const On, spinor *const E, spinor *const O) {
  apply2(ses.refresh(true), En, On, E, O, [&](Ctx c, Fld fen, Fld fon, Fld fe, Fld fo) {
    CK(tmhip_H_eo_tm_inv_psi(c, fen, fo, TMHIP_EO, +1.));
    CK(tmhip_H_eo_tm_inv_psi(c, fon, fe, TMHIP_OE, +1.));
  });
}

// ------------------------------------------------------------------ non-degenerate doublet (tm_operators_nd.c)
ND_OP(Qtm_ndpsi, tmhip_Qtm_ndpsi)                /* tm_operators_nd.c:68-89 */
ND_OP(Qtm_dagger_ndpsi, tmhip_Qtm_dagger_ndpsi)  /* :130-152 */
ND_OP(Qtm_pm_ndpsi, tmhip_Qtm_pm_ndpsi)          /* :195-238 */
void Q_tau1_sub_const_ndpsi(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c, const _Complex double z, const double Cpol,
                            const double invev) {   /* :311-380 */
  apply2(ses.refresh_nd("Q_tau1_sub_const_ndpsi"), l_s, l_c, k_s, k_c, [&](Ctx c, Fld fls, Fld flc, Fld fks, Fld fkc) {
    CK(tmhip_Q_tau1_sub_const_ndpsi(c, fls, flc, fks, fkc, __real__ z, __imag__ z, Cpol, invev));
  });
}
void M_ee_inv_ndpsi(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c, const double mu, const double eps) {   /* :639-696 */
  apply2(ses.refresh_nd("M_ee_inv_ndpsi"), l_s, l_c, k_s, k_c, [&](Ctx c, Fld fls, Fld flc, Fld fks, Fld fkc) { CK(tmhip_M_ee_inv_ndpsi(c, fls, flc, fks, fkc, mu, eps)); });
}
void H_eo_tm_ndpsi(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c, const int ieo) {   /* :508-519 */
  apply2(ses.refresh_nd("H_eo_tm_ndpsi"), l_s, l_c, k_s, k_c, [&](Ctx c, Fld fls, Fld flc, Fld fks, Fld fkc) { CK(tmhip_H_eo_tm_ndpsi(c, fls, flc, fks, fkc, ieo)); });
}
/* :582-597, the same sequence of add / diff / mul_r (so p or q may be r or s exactly as in the reference) */
void mul_one_pm_itau2(spinor *const p, spinor *const q, spinor *const r, spinor *const s, const double sign, const int N) {
  tmhip_ctx *c = ses.refresh(false);
  if (N == 0) return;
  if (N < 0 || N > VOLUME / 2) die("mul_one_pm_itau2: N must be in [0, VOLUME/2]");
  tmhip_field *fr = in(c, r, TMHIP_FIELD_EO, N), *fs = in(c, s, TMHIP_FIELD_EO, N);
  tmhip_field *fp = out(c, p, TMHIP_FIELD_EO, N), *fq = out(c, q, TMHIP_FIELD_EO, N);
  const double fac = 1. / sqrt(2.);
  if (sign > 0) { CK(tmhip_add(c, fp, fr, fs, N)); CK(tmhip_diff(c, fq, fs, fr, N)); }
  else { CK(tmhip_diff(c, fp, fr, fs, N)); CK(tmhip_add(c, fq, fr, fs, N)); }
  CK(tmhip_mul_r(c, fp, fac, fp, N));
  CK(tmhip_mul_r(c, fq, fac, fq, N));
  done(c, p); done(c, q);
}

// ------------------------------------------------------------------ clover twisted mass
void tmlqcd_hip_update_clover(void) { ses.clover_stale(); }
/* sw_term(g_gauge_field, kappa, c_sw) (operator/clover_term.c:88) computed in HBM; the host's sw array, if the program
 * has one (init_sw_fields), receives a copy so that host-side consumers (the reference's sw_deriv ...) keep working. */
void tmlqcd_hip_sw_term(const double kappa, const double c_sw) {
  tmhip_ctx *c = ses.refresh(false);
  CK(tmhip_sw_term(c, &g_gauge_field[0][0], kappa, c_sw));
  if (&sw && sw) CK(tmhip_get_clover(c, &sw[0][0][0], nullptr));
  ses.clover_uploaded = false;
  ses.sw_on_device = true;
}
/* sw_invert(ieo, mu) (operator/clover_invert.c:170) from the device-resident clover term */
void tmlqcd_hip_sw_invert(const int ieo, const double mu) {
  tmhip_ctx *c = ses.refresh(false);
  CK(tmhip_sw_invert(c, ieo, mu));
  if (&sw_inv && sw_inv) CK(tmhip_get_clover(c, nullptr, &sw_inv[0][0][0]));
  ses.clover_uploaded = true;   // the device copy is the fresh one
}
EO_OP(Qsw_pm_psi, ses.refresh_clover(), tmhip_Qsw_pm_psi)      /* clovertm_operators.c:233-245 */
EO_OP(Msw_plus_psi, ses.refresh_clover(), tmhip_Msw_plus_psi)  /* clovertm_operators.c:256-261 */
EO_OP(Qsw_psi, ses.refresh_clover(), tmhip_Qsw_psi)              /* :201-206 */
EO_OP(Qsw_minus_psi, ses.refresh_clover(), tmhip_Qsw_minus_psi)  /* :209-214 */
EO_OP(Qsw_plus_psi, ses.refresh_clover(), tmhip_Qsw_plus_psi)    /* :217-222 */
EO_OP(Qsw_sq_psi, ses.refresh_clover(), tmhip_Qsw_sq_psi)        /* :225-237 */
EO_OP(Msw_psi, ses.refresh_clover(), tmhip_Msw_psi)              /* :247-252 */
EO_OP(Msw_minus_psi, ses.refresh_clover(), tmhip_Msw_minus_psi)  /* :261-266 */
/* clovertm_operators.c:96-110 */
void Msw_full(spinor *const En, spinor *const On, spinor *const E, spinor *const O) {
  apply2(ses.refresh_clover(), En, On, E, O, [&](Ctx c, Fld fen, Fld fon, Fld fe, Fld fo) { CK(tmhip_Msw_full(c, fen, fon, fe, fo)); });
}
/* operator/assign_mul_one_sw_pm_imu_inv_block_body.c:1-72 */
void assign_mul_one_sw_pm_imu(const int ieo, spinor *const k, spinor *const l, const double mu) {
  apply(ses.refresh_clover(), TMHIP_FIELD_EO, k, l, nullptr, [&](Ctx c, Fld fk, Fld fl, Fld) { CK(tmhip_assign_mul_one_sw_pm_imu(c, ieo, fk, fl, mu)); });
}
/* operator/assign_mul_one_sw_pm_imu_inv_block_body.c:143-196 (ieo and mu are not looked at, as in the reference) */
void assign_mul_one_sw_pm_imu_inv(const int ieo, spinor *const k, spinor *const l, const double mu) {
  apply(ses.refresh_clover(), TMHIP_FIELD_EO, k, l, nullptr, [&](Ctx c, Fld fk, Fld fl, Fld) { CK(tmhip_assign_mul_one_sw_pm_imu_inv(c, ieo, fk, fl, mu)); });
}
/* clovertm_operators.c:873-940, 1098-1140: the even-site forms of the two above */
void Mee_sw_psi(spinor *const k, spinor *const l, const double mu) { assign_mul_one_sw_pm_imu(0, k, l, mu); }
void Mee_sw_inv_psi(spinor *const k, spinor *const l, const double mu) { assign_mul_one_sw_pm_imu_inv(0, k, l, mu); }
/* clovertm_operators.c:268-272 */
void H_eo_sw_inv_psi(spinor *const l, spinor *const k, const int ieo, const int tau3sign, const double mu) {
  apply(ses.refresh_clover(), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { CK(tmhip_H_eo_sw_inv_psi(c, fl, fk, ieo, tau3sign, mu)); });
}
/* clovertm_operators.c:287-350 (in place) */
void clover_inv(spinor *const l, const int tau3sign, const double mu) {
  tmhip_ctx *c = ses.refresh_clover();
  tmhip_field *fl = in(c, l, TMHIP_FIELD_EO);
  CK(tmhip_clover_inv(c, fl, tau3sign, mu));
  done(c, l);
}
/* clovertm_operators.c:448-520 */
void clover_gamma5(const int ieo, spinor *const l, const spinor *const k, const spinor *const j, const double mu) {
  apply(ses.refresh_clover(), TMHIP_FIELD_EO, l, k, j, [&](Ctx c, Fld fl, Fld fk, Fld fj) { CK(tmhip_clover_gamma5(c, ieo, fl, fk, fj, mu)); });
}
/* clovertm_operators.c:535-600 */
void clover(const int ieo, spinor *const l, const spinor *const k, const spinor *const j, const double mu) {
  apply(ses.refresh_clover(), TMHIP_FIELD_EO, l, k, j, [&](Ctx c, Fld fl, Fld fk, Fld fj) { CK(tmhip_clover(c, ieo, fl, fk, fj, mu)); });
}

// ------------------------------------------------------------------ clover doublet (Qsw_*_ndpsi, tm_operators_nd.c; clovertm_operators.c)
// The core refuses, with a message, when the device's 1+T or sw_inv_nd do not belong to the current links: run tmlqcd_hip_sw_term (or
// the host's sw_term + tmlqcd_hip_update_clover) and sw_invert_nd first, as ndrat_monomial.c:89-91 does.
/* operator/clover_invert.c:440 sw_invert_nd(mshift) from the device's clover term (the host's sw goes up first when the device has none
 * for these links); the host's sw_inv, when the program has one, receives the result in its first VOLUME/2 entries as in the reference.
 * On the device it lives beside sw_inv, not in it. */
void sw_invert_nd(const double mshift) {
  tmhip_ctx *c = ses.refresh(false);
  if (!ses.sw_on_device) { ses.clover_uploaded = false; ses.ensure_clover(); }
  CK(tmhip_sw_invert_nd(c, mshift));
  if (&sw_inv && sw_inv) CK(tmhip_get_clover_nd(c, &sw_inv[0][0][0]));
}
/* near-singular pivots met by the last sw_invert_nd / tmlqcd_hip_sw_invert (what the reference prints as "inversion failed in six_invert") */
int tmlqcd_hip_sw_invert_failures(void) {
  int n = 0;
  CK(tmhip_sw_invert_failures(ctx(), &n));
  return n;
}
/* operator/clover_det.c:115 sw_trace(ieo, mu) and :202 sw_trace_nd(ieo, mu, eps): the tr-log energies of clover_trlog_monomial.c,
 * clovernd_trlog_monomial.c and the trlog option of the clover monomials, from the device's clover term where it belongs to the current
 * links (the host's sw goes up first otherwise, as for sw_invert_nd).  On T-split ranks the sum over all ranks, as the reference's. */
double sw_trace(const int ieo, const double mu) {
  tmhip_ctx *c = ses.refresh(false);
  if (!ses.sw_on_device) { ses.clover_uploaded = false; ses.ensure_clover(); }
  double r = 0.0;
  CK(tmhip_sw_trace(c, ieo, mu, g_nproc_t > 1, &r));
  return r;
}
double sw_trace_nd(const int ieo, const double mu, const double eps) {
  tmhip_ctx *c = ses.refresh(false);
  if (!ses.sw_on_device) { ses.clover_uploaded = false; ses.ensure_clover(); }
  double r = 0.0;
  CK(tmhip_sw_trace_nd(c, ieo, mu, eps, g_nproc_t > 1, &r));
  return r;
}
/* pivots below tiny_t met by the last sw_trace / sw_trace_nd (what the reference prints as "ifail > 0 in six_det") */
int tmlqcd_hip_sw_trace_failures(void) { return tmhip_sw_trace_failures(ctx()); }
/* operator/clover_deriv.c:156 sw_deriv_nd(ieo) into the device-resident swm / swp (tmlqcd_hip_swpm_zero / tmlqcd_hip_sw_all) */
void sw_deriv_nd(const int ieo) { CK(tmhip_sw_deriv_nd(ses.refresh(false), ieo)); }
ND_OP(Qsw_ndpsi, tmhip_Qsw_ndpsi)                /* tm_operators_nd.c:91-111 */
ND_OP(Qsw_dagger_ndpsi, tmhip_Qsw_dagger_ndpsi)  /* :154-174 */
ND_OP(Qsw_pm_ndpsi, tmhip_Qsw_pm_ndpsi)          /* :240-285 */
ND_OP(H_eo_sw_ndpsi, tmhip_H_eo_sw_ndpsi)        /* :521-535 */
ND_OP(Msw_ee_inv_ndpsi, tmhip_Msw_ee_inv_ndpsi)  /* :539-549 */
void Qsw_tau1_sub_const_ndpsi(spinor *const l_s, spinor *const l_c, spinor *const k_s, spinor *const k_c, const _Complex double z, const double Cpol,
                              const double invev) {   /* :378-444 */
  apply2(ses.refresh_nd("Qsw_tau1_sub_const_ndpsi"), l_s, l_c, k_s, k_c, [&](Ctx c, Fld fls, Fld flc, Fld fks, Fld fkc) {
    CK(tmhip_Qsw_tau1_sub_const_ndpsi(c, fls, flc, fks, fkc, __real__ z, __imag__ z, Cpol, invev));
  });
}
/* clovertm_operators.c:960-1074 */
void assign_mul_one_sw_pm_imu_eps(const int ieo, spinor *const k_s, spinor *const k_c, const spinor *const l_s, const spinor *const l_c,
                                  const double mu, const double eps) {
  apply2(ses.refresh_nd("assign_mul_one_sw_pm_imu_eps"), k_s, k_c, l_s, l_c, [&](Ctx c, Fld fks, Fld fkc, Fld fls, Fld flc) {
    CK(tmhip_assign_mul_one_sw_pm_imu_eps(c, ieo, fks, fkc, fls, flc, mu, eps));
  });
}
/* clovertm_operators.c:352-425, in place */
void clover_inv_nd(const int ieo, spinor *const l_c, spinor *const l_s) {
  tmhip_ctx *c = ses.refresh_nd("clover_inv_nd");
  tmhip_field *flc = in(c, l_c, TMHIP_FIELD_EO), *fls = in(c, l_s, TMHIP_FIELD_EO);
  CK(tmhip_clover_inv_nd(c, ieo, flc, fls));
  done(c, l_c); done(c, l_s);
}
/* clovertm_operators.c:733-850 */
void clover_gamma5_nd(const int ieo, spinor *const l_c, spinor *const l_s, const spinor *const k_c, const spinor *const k_s,
                      const spinor *const j_c, const spinor *const j_s, const double mubar, const double epsbar) {
  tmhip_ctx *c = ses.refresh_nd("clover_gamma5_nd");
  tmhip_field *fkc = in(c, k_c, TMHIP_FIELD_EO), *fks = in(c, k_s, TMHIP_FIELD_EO), *fjc = in(c, j_c, TMHIP_FIELD_EO), *fjs = in(c, j_s, TMHIP_FIELD_EO);
  tmhip_field *flc = out(c, l_c, TMHIP_FIELD_EO), *fls = out(c, l_s, TMHIP_FIELD_EO);
  CK(tmhip_clover_gamma5_nd(c, ieo, flc, fls, fkc, fks, fjc, fjs, mubar, epsbar));
  done(c, l_c); done(c, l_s);
}

// ------------------------------------------------------------------ site-diagonal ops
/* mul_one_pm_imu_inv_body.c:1-41 */
void mul_one_pm_imu_inv(spinor *const l, const double _sign, const int N) {
  lin_op(N, rw(l), none(), none(), [&](Ctx c, Fld fl, Fld, Fld, int n) { CK(tmhip_mul_one_pm_imu_inv(c, fl, _sign, n)); });
}
/* mul_one_pm_imu_inv_body.c:43-80 */
void assign_mul_one_pm_imu_inv(spinor *const l, spinor *const k, const double _sign, const int N) {
  lin_op(N, rd(k), wr(l), none(), [&](Ctx c, Fld fk, Fld fl, Fld, int n) { CK(tmhip_assign_mul_one_pm_imu_inv(c, fl, fk, _sign, n)); });
}
/* tm_operators.c:669-720 */
void assign_mul_one_pm_imu(spinor *const l, spinor *const k, const double _sign, const int N) {
  lin_op(N, rd(k), wr(l), none(), [&](Ctx c, Fld fk, Fld fl, Fld, int n) { CK(tmhip_assign_mul_one_pm_imu(c, fl, fk, _sign, n)); });
}
/* tm_operators.c:627-667 */
void mul_one_pm_imu(spinor *const l, const double _sign) {
  tmhip_ctx *c = ses.refresh(false);
  tmhip_field *fl = in(c, l, TMHIP_FIELD_EO);
  CK(tmhip_mul_one_pm_imu(c, fl, _sign));
  done(c, l);
}
/* mul_one_pm_imu_sub_mul_body.c:1-48 */
void mul_one_pm_imu_sub_mul(spinor *const l, spinor *const k, spinor *const j, const double _sign, const int N) {
  lin_op(N, rd(k), rd(j), wr(l), [&](Ctx c, Fld fk, Fld fj, Fld fl, int n) { CK(tmhip_mul_one_pm_imu_sub_mul(c, fl, fk, fj, _sign, n)); });
}
/* tm_operators.c:813-858 */
void mul_one_pm_imu_sub_mul_gamma5(spinor *const l, spinor *const k, spinor *const j, const double _sign) {
  apply(ses.refresh(false), TMHIP_FIELD_EO, l, k, j, [&](Ctx c, Fld fl, Fld fk, Fld fj) { CK(tmhip_mul_one_pm_imu_sub_mul_gamma5(c, fl, fk, fj, _sign)); });
}
/* tm_operators.c:781-810 (external linkage in the reference although no header declares it) */
void mul_one_sub_mul_gamma5(spinor *const l, spinor *const k, spinor *const j) {
  apply(ses.refresh(false), TMHIP_FIELD_EO, l, k, j, [&](Ctx c, Fld fl, Fld fk, Fld fj) { CK(tmhip_mul_one_sub_mul_gamma5(c, fl, fk, fj)); });
}
/* tm_operators.c:723-775: l = (1 + i mu g5) k with an explicit mu */
void Mee_psi(spinor *const l, spinor *const k, const double mu) {
  apply(ses.refresh(false), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    with_mu(c, mu, [&] { CK(tmhip_assign_mul_one_pm_imu(c, fl, fk, +1., VOLUME / 2)); });
  });
}
/* tm_operators.c:587-625: l = (1 - i mu g5)/(1+mu^2) k with an explicit mu */
void Mee_inv_psi(spinor *const l, spinor *const k, const double mu) {
  apply(ses.refresh(false), TMHIP_FIELD_EO, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    with_mu(c, mu, [&] { CK(tmhip_assign_mul_one_pm_imu_inv(c, fl, fk, +1., VOLUME / 2)); });
  });
}
/* gamma.c:77-98 */
void gamma5(spinor *const l, spinor *const k, const int V) {
  lin_op(V, rd(k), wr(l), none(), [&](Ctx c, Fld fk, Fld fl, Fld, int n) { CK(tmhip_gamma5(c, fl, fk, n)); });
}

// ------------------------------------------------------------------ full-lattice operators
/* The reference toggles g_mu's sign around D_psi (tm_operators.c:380-492); refresh() re-reads it. */
/* tm_operators.c:111-114 */
void Q_psi(spinor *const P, spinor *const Q) {
  apply(ses.refresh(true), TMHIP_FIELD_FULL, P, Q, nullptr, [&](Ctx c, Fld fp, Fld fq, Fld) { d_psi_core(c, fp, fq); g5_full(c, fp, fp); });
}
/* tm_operators.c:486-490 */
void Q_plus_psi(spinor *const l, spinor *const k) { Q_psi(l, k); }
/* tm_operators.c:460-466 */
void Q_minus_psi(spinor *const l, spinor *const k) {
  apply(ses.refresh(true), TMHIP_FIELD_FULL, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    with_mu(c, -g_mu, [&] { d_psi_core(c, fl, fk); });
    g5_full(c, fl, fl);
  });
}
/* tm_operators.c:468-473 */
void M_minus_psi(spinor *const l, spinor *const k) {
  apply(ses.refresh(true), TMHIP_FIELD_FULL, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) { with_mu(c, -g_mu, [&] { d_psi_core(c, fl, fk); }); });
}
/* tm_operators.c:380-388 : Q_+ Q_- on the full lattice */
void Q_pm_psi(spinor *const l, spinor *const k) { q_pm_full(l, k, -g_mu); }
/* tm_operators.c:453-461 : Q_pm_psi with the first twist scaled by 10 (mu -> -10 mu, then +mu) */
void Q_pm_psi2(spinor *const l, spinor *const k) { q_pm_full(l, k, -10. * g_mu); }
/* tm_operators.c:402-436 : Q_pm_psi with spinorPrecondition() (solver/dirac_operator_eigenvectors.c, FFTW-based, stays in
 * tmLQCD) applied before, between and after the two D_psi where g_prec_sequence_d_dagger_d[] is non-zero.  Host-level
 * composition over this library's own assign / D_psi / gamma5; the preconditioner and its globals are weak references, so a host
 * program that does not link them still resolves this symbol and gets the unpreconditioned sequence. */
void Q_pm_psi_prec(spinor *const l, spinor *const k) {
  double seq[3] = {0., 0., 0.};
  if (g_prec_sequence_d_dagger_d) for (int i = 0; i < 3; i++) seq[i] = g_prec_sequence_d_dagger_d[i];
  const bool any = seq[0] != 0. || seq[1] != 0. || seq[2] != 0.;
  if (any && (!spinorPrecondition || !&g_precWS || !&L))
    die("Q_pm_psi_prec: g_prec_sequence_d_dagger_d is set but spinorPrecondition (solver/dirac_operator_eigenvectors.c) is not linked");
  static spinor *tmp = nullptr;
  static int tmp_sites = 0;
  if (tmp_sites < VOLUMEPLUSRAND) {
    free(tmp);
    tmp = (spinor *)malloc((size_t)VOLUMEPLUSRAND * sizeof(spinor));
    if (!tmp) die("Q_pm_psi_prec: out of host memory");
    tmp_sites = VOLUMEPLUSRAND;
  }
  auto prec = [&](spinor *out_, const spinor *in_, double a) {
    TM_COMPLEX alpha = a;
    spinorPrecondition(out_, in_, g_precWS, T, L, alpha, 0, 1);
    tmlqcd_hip_host_modified(out_);
  };
  if (seq[0] != 0.) { tmlqcd_hip_sync_to_host(k); prec(l, k, seq[0]); } else assign(l, k, VOLUME);
  g_mu = -g_mu;
  D_psi(tmp, l);
  gamma5(l, tmp, VOLUME);
  g_mu = -g_mu;
  if (seq[1] != 0.) { tmlqcd_hip_sync_to_host(l); prec(l, l, seq[1]); }
  D_psi(tmp, l);
  gamma5(l, tmp, VOLUME);
  if (seq[2] != 0.) { tmlqcd_hip_sync_to_host(l); prec(l, l, seq[2]); }
}
/* tm_operators.c:440-449 : "version for the gpu", gamma5 applied to the INPUT in place first, none at the end */
void Q_pm_psi_gpu(spinor *const l, spinor *const k) {
  tmhip_ctx *c = ses.refresh(true);
  tmhip_field *fk = in(c, k, TMHIP_FIELD_FULL), *fl = out(c, l, TMHIP_FIELD_FULL), *tmp = full_tmp(c);
  g5_full(c, fk, fk);
  with_mu(c, -g_mu, [&] { d_psi_core(c, fl, fk); g5_full(c, tmp, fl); });
  d_psi_core(c, fl, tmp);
  done(c, k); done(c, l);
}
/* tm_operators.c:476-483 */
void Q_minus_psi_gpu(spinor *const l, spinor *const k) {
  tmhip_ctx *c = ses.refresh(true);
  tmhip_field *fk = in(c, k, TMHIP_FIELD_FULL), *fl = out(c, l, TMHIP_FIELD_FULL);
  g5_full(c, fk, fk);
  with_mu(c, -g_mu, [&] { d_psi_core(c, fl, fk); });
  g5_full(c, fl, fl);
  done(c, k); done(c, l);
}
/* tm_operators.c:390-397 */
void D_dagg_psi(spinor *const l, spinor *const k) {
  apply(ses.refresh(true), TMHIP_FIELD_FULL, l, k, nullptr, [&](Ctx c, Fld fl, Fld fk, Fld) {
    tmhip_field *tmp = full_tmp(c);
    g5_full(c, fl, fk);
    with_mu(c, -g_mu, [&] { d_psi_core(c, tmp, fl); });
    g5_full(c, fl, tmp);
  });
}

// ------------------------------------------------------------------ linalg
/* linalg/square_norm.c:253-320 */
double square_norm(const spinor *const P, const int N, const int parallel) {
  double res = 0;
  lin_op(N, rd(P), none(), none(), [&](Ctx c, Fld fp, Fld, Fld, int n) { double r; CK(tmhip_square_norm(c, fp, n, parallel, &r)); res += r; });
  return res;
}
/* linalg/scalar_prod_r.c:135-197 */
double scalar_prod_r(const spinor *const S, const spinor *const R, const int N, const int parallel) {
  double res = 0;
  lin_op(N, rd(S), rd(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { double r; CK(tmhip_scalar_prod_r(c, fs, fr, n, parallel, &r)); res += r; });
  return res;
}
/* linalg/assign_add_mul_r.c:346-381 */
void assign_add_mul_r(spinor *const P, spinor *const Q, const double cc, const int N) {
  lin_op(N, rw(P), rd(Q), none(), [&](Ctx c, Fld fp, Fld fq, Fld, int n) { CK(tmhip_assign_add_mul_r(c, fp, fq, cc, n)); });
}
/* linalg/assign_add_mul.c: P += c Q, complex c */
void assign_add_mul(spinor *const P, spinor *const Q, const _Complex double cc, const int N) {
  lin_op(N, rw(P), rd(Q), none(), [&](Ctx c, Fld fp, Fld fq, Fld, int n) { CK(tmhip_assign_add_mul(c, fp, fq, __real__ cc, __imag__ cc, n)); });
}
/* linalg/assign_mul_add_r.c:340-377 */
void assign_mul_add_r(spinor *const R, const double cc, const spinor *const S, const int N) {
  lin_op(N, rw(R), rd(S), none(), [&](Ctx c, Fld fr, Fld fs, Fld, int n) { CK(tmhip_assign_mul_add_r(c, fr, cc, fs, n)); });
}
/* linalg/assign_mul_add_r_and_square.c:145-213 */
double assign_mul_add_r_and_square(spinor *const R, const double cc, const spinor *const S, const int N, const int parallel) {
  double res = 0;
  lin_op(N, rw(R), rd(S), none(), [&](Ctx c, Fld fr, Fld fs, Fld, int n) {
    double r;
    CK(tmhip_assign_mul_add_r_and_square(c, fr, cc, fs, n, parallel, &r));
    res += r;
  });
  return res;
}
/* linalg/diff.c:270-309 */
void diff(spinor *const Q, const spinor *const R, const spinor *const S, const int N) {
  lin_op(N, rd(R), rd(S), wr(Q), [&](Ctx c, Fld fr, Fld fs, Fld fq, int n) { CK(tmhip_diff(c, fq, fr, fs, n)); });
}
/* linalg/add.c:45-80 */
void add(spinor *const Q, const spinor *const R, const spinor *const S, const int N) {
  lin_op(N, rd(R), rd(S), wr(Q), [&](Ctx c, Fld fr, Fld fs, Fld fq, int n) { CK(tmhip_add(c, fq, fr, fs, n)); });
}
/* linalg/mul_r.c:40-75 */
void mul_r(spinor *const R, const double cc, spinor *const S, const int N) {
  lin_op(N, rd(S), wr(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { CK(tmhip_mul_r(c, fr, cc, fs, n)); });
}
/* linalg/scalar_prod.c: sum conj(S) R */
_Complex double scalar_prod(const spinor *const S, const spinor *const R, const int N, const int parallel) {
  double re = 0, im = 0;
  lin_op(N, rd(S), rd(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { double r[2]; CK(tmhip_scalar_prod(c, fs, fr, n, parallel, r)); re += r[0]; im += r[1]; });
  _Complex double res;
  __real__ res = re; __imag__ res = im;
  return res;
}
/* linalg/assign_diff_mul.c: S -= c R */
void assign_diff_mul(spinor *const S, spinor *const R, const _Complex double cc, const int N) {
  lin_op(N, rw(S), rd(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { CK(tmhip_assign_diff_mul(c, fs, fr, __real__ cc, __imag__ cc, n)); });
}
/* linalg/mul.c: R = c S */
void mul(spinor *const R, const _Complex double cc, spinor *const S, const int N) {
  lin_op(N, rd(S), wr(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { CK(tmhip_mul(c, fr, __real__ cc, __imag__ cc, fs, n)); });
}
/* linalg/assign_add_mul_add_mul.c:42-60: R += c1 S + c2 U */
void assign_add_mul_add_mul(spinor *const R, spinor *const S, spinor *const U, const _Complex double c1, const _Complex double c2, const int N) {
  lin_op(N, rw(R), rd(S), rd(U), [&](Ctx c, Fld fr, Fld fs, Fld fu, int n) {
    CK(tmhip_assign_add_mul_add_mul(c, fr, fs, fu, __real__ c1, __imag__ c1, __real__ c2, __imag__ c2, n));
  });
}
/* linalg/assign_mul_bra_add_mul_ket_add.c:44-63: R = c2 (R + c1 S) + U */
void assign_mul_bra_add_mul_ket_add(spinor *const R, spinor *const S, spinor *const U, const _Complex double c1, const _Complex double c2, const int N) {
  lin_op(N, rw(R), rd(S), rd(U), [&](Ctx c, Fld fr, Fld fs, Fld fu, int n) {
    CK(tmhip_assign_mul_bra_add_mul_ket_add(c, fr, fs, fu, __real__ c1, __imag__ c1, __real__ c2, __imag__ c2, n));
  });
}
/* linalg/assign.c:42-46 */
void assign(spinor *const R, spinor *const S, const int N) {
  lin_op(N, rd(S), wr(R), none(), [&](Ctx c, Fld fs, Fld fr, Fld, int n) { CK(tmhip_assign(c, fr, fs, n)); });
}

/* fp32 instances of the site-diagonal twists (tm_operators.c:8-47 -> mul_one_pm_imu_inv_body.c, mul_one_pm_imu_sub_mul_body.c);
 * callers hand over domain blocks of any length (solver/Msap.c:409-418), so these go through a staging buffer, not the registry */
void mul_one_pm_imu_inv_32(spinor32 *const l, const double _sign, const int N) {
  tmhip_ctx *c = ses.refresh(false);
  const float nrm = (float)(1. / (1. + g_mu * g_mu));
  CK(tmhip_diag32_host(c, l, l, nullptr, nrm, (_sign < 0. ? 1. : -1.) * nrm * g_mu, N));
}
void assign_mul_one_pm_imu_inv_32(spinor32 *const l, spinor32 *const k, const double _sign, const int N) {
  tmhip_ctx *c = ses.refresh(false);
  const float nrm = (float)(1. / (1. + g_mu * g_mu));
  CK(tmhip_diag32_host(c, l, k, nullptr, nrm, (_sign < 0. ? 1. : -1.) * nrm * g_mu, N));
}
void mul_one_pm_imu_sub_mul_32(spinor32 *const l, spinor32 *const k, spinor32 *const j, const double _sign, const int N) {
  tmhip_ctx *c = ses.refresh(false);
  CK(tmhip_diag32_host(c, l, k, j, 1., (_sign < 0. ? -1. : 1.) * g_mu, N));
}

// ------------------------------------------------------------------ fp32 twins on host spinor32 arrays
// Hopping_Matrix_32 (operator/Hopping_Matrix_32.c:97-127), Qtm_pm_psi_32 (operator/tm_operators_32.c:94-112) and the fp32 linalg
// (linalg/*_32.c) by their reference names.  Host spinor32 arrays are not kept in the registry (the solvers that iterate in fp32 --
// mixed_cg_her, rg_mixed_cg_her -- run device-resident through their own entry points below): every call copies its operands in and its
// result out through a small pool of device fields, i.e. the coherent semantics of the fp64 symbols, PCIe-bound and exact.
// The `_orphaned` convention (SURVEY 8b "Threading"): the reference's fp32 operators are called INSIDE an enclosing OpenMP parallel
// region by all its threads (Qtm_pm_psi_32 opens the region, operator/tm_operators_32.c:96-110).  Here ONE thread issues the device
// call and all threads of the team meet before and after it -- orphaned `omp barrier` / `omp master`, which bind to whatever
// region encloses the call and are no-ops outside of one (this file is compiled with -fopenmp).
void Hopping_Matrix_32(const int ieo, spinor32 *const l, spinor32 *const k) {   /* called from the master thread outside any parallel region */
  tmhip_ctx *c = ses.refresh(true);
  if ((void *)l == (void *)k) die("Hopping_Matrix_32: l and k must differ");
  tmhip_field *fk = in32(c, 0, k, VOLUME / 2), *fl = f32(c, 1);
  CK(tmhip_hopping_matrix_32(c, ieo, fl, fk));
  CK(tmhip_field_download32(c, fl, l, VOLUME / 2));
}
void Hopping_Matrix_32_orphaned(const int ieo, spinor32 *const l, spinor32 *const k) {   /* by every thread of the enclosing team */
  team_once([&] { Hopping_Matrix_32(ieo, l, k); });
}
void Qtm_pm_psi_32(spinor32 *const l, spinor32 *const k) {
  tmhip_ctx *c = ses.refresh(true);
  tmhip_field *fk = in32(c, 0, k, VOLUME / 2), *fl = f32(c, 1);
  CK(tmhip_Qtm_pm_psi_32(c, fl, fk));
  CK(tmhip_field_download32(c, fl, l, VOLUME / 2));
}
// The fp32 doublet (operator/tm_operators_nd_32.c): inputs in pool fields 0..3, outputs in 4, 5, so l may be k or j as in the reference
void Qtm_pm_ndpsi_32(spinor32 *const l_s, spinor32 *const l_c, spinor32 *const k_s, spinor32 *const k_c) {   /* :215-263 */
  tmhip_ctx *c = ses.refresh_nd("Qtm_pm_ndpsi_32");
  tmhip_field *fks = in32(c, 0, k_s, VOLUME / 2), *fkc = in32(c, 1, k_c, VOLUME / 2), *fls = f32(c, 4), *flc = f32(c, 5);
  CK(tmhip_Qtm_pm_ndpsi_32(c, fls, flc, fks, fkc));
  CK(tmhip_field_download32(c, fls, l_s, VOLUME / 2));
  CK(tmhip_field_download32(c, flc, l_c, VOLUME / 2));
}
void M_ee_inv_ndpsi_32(spinor32 *const l_s, spinor32 *const l_c, spinor32 *const k_s, spinor32 *const k_c, const float mu, const float eps) {   /* :137-149 */
  tmhip_ctx *c = ses.refresh_nd("M_ee_inv_ndpsi_32");
  tmhip_field *fks = in32(c, 0, k_s, VOLUME / 2), *fkc = in32(c, 1, k_c, VOLUME / 2), *fls = f32(c, 4), *flc = f32(c, 5);
  CK(tmhip_M_ee_inv_ndpsi_32(c, fls, flc, fks, fkc, mu, eps));
  CK(tmhip_field_download32(c, fls, l_s, VOLUME / 2));
  CK(tmhip_field_download32(c, flc, l_c, VOLUME / 2));
}
void M_oo_sub_g5_ndpsi_32(spinor32 *const l_s, spinor32 *const l_c, spinor32 *const k_s, spinor32 *const k_c, spinor32 *const j_s,
                          spinor32 *const j_c, const float mu, const float eps) {   /* :200-213 */
  tmhip_ctx *c = ses.refresh_nd("M_oo_sub_g5_ndpsi_32");
  tmhip_field *fks = in32(c, 0, k_s, VOLUME / 2), *fkc = in32(c, 1, k_c, VOLUME / 2), *fjs = in32(c, 2, j_s, VOLUME / 2), *fjc = in32(c, 3, j_c, VOLUME / 2);
  tmhip_field *fls = f32(c, 4), *flc = f32(c, 5);
  CK(tmhip_M_oo_sub_g5_ndpsi_32(c, fls, flc, fks, fkc, fjs, fjc, mu, eps));
  CK(tmhip_field_download32(c, fls, l_s, VOLUME / 2));
  CK(tmhip_field_download32(c, flc, l_c, VOLUME / 2));
}
float square_norm_32(const spinor32 *const P, const int N, const int parallel) {   /* linalg/square_norm_32.c:95 */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "square_norm_32");
  if (N == 0) return 0.f;
  double r = 0;
  CK(tmhip_square_norm_32(c, in32(c, 0, P, N), N, parallel, &r));
  return (float)r;
}
float scalar_prod_r_32(const spinor32 *const S, const spinor32 *const R, const int N, const int parallel) {   /* linalg/scalar_prod_r_32.c:109 */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "scalar_prod_r_32");
  if (N == 0) return 0.f;
  double r = 0;
  tmhip_field *fs = in32(c, 0, S, N), *fr = (const void *)S == (const void *)R ? fs : in32(c, 1, R, N);
  CK(tmhip_scalar_prod_r_32(c, fs, fr, N, parallel, &r));
  return (float)r;
}
void assign_add_mul_r_32(spinor32 *const R, spinor32 *const S, const float cc, const int N) {   /* linalg/assign_add_mul_r_32.c:104: R += c S */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "assign_add_mul_r_32");
  if (N == 0) return;
  tmhip_field *fr = in32(c, 0, R, N), *fs = (void *)S == (void *)R ? fr : in32(c, 1, S, N);
  CK(tmhip_assign_add_mul_r_32(c, fr, fs, cc, N));
  CK(tmhip_field_download32(c, fr, R, N));
}
void assign_mul_add_r_32(spinor32 *const R, const float cc, const spinor32 *const S, const int N) {   /* linalg/assign_mul_add_r_32.c:81: R = c R + S */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "assign_mul_add_r_32");
  if (N == 0) return;
  tmhip_field *fr = in32(c, 0, R, N), *fs = (const void *)S == (const void *)R ? fr : in32(c, 1, S, N);
  CK(tmhip_assign_mul_add_r_32(c, fr, cc, fs, N));
  CK(tmhip_field_download32(c, fr, R, N));
}
void diff_32(spinor32 *const Q, const spinor32 *const R, const spinor32 *const S, const int N) {   /* linalg/diff_32.c:39: Q = R - S */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "diff_32");
  if (N == 0) return;
  tmhip_field *fq = in32(c, 0, S, N), *fr = in32(c, 1, R, N);     // Q = -1 * S + R
  CK(tmhip_assign_mul_add_r_32(c, fq, -1.f, fr, N));
  CK(tmhip_field_download32(c, fq, Q, N));
}
void assign_to_32(spinor32 *const R, spinor *const S, const int N) {   /* linalg/assign_to_32.c:37: the fp64 operand goes through the registry like any other input */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "assign_to_32");
  if (N == 0) return;
  tmhip_field *fs = in(c, S, TMHIP_FIELD_EO), *fr = f32(c, 0);
  CK(tmhip_assign_to_32(c, fr, fs, N));
  CK(tmhip_field_download32(c, fr, R, N));
}
void assign_to_64(spinor *const R, spinor32 *const S, const int N) {   /* linalg/assign_to_32.c:84 */
  tmhip_ctx *c = ses.refresh(false);
  need_N32(N, "assign_to_64");
  if (N == 0) return;
  if (N != VOLUME / 2) die("assign_to_64: N must be VOLUME/2 (the fp64 result is a registered one-parity field)");
  tmhip_field *fs = in32(c, 0, S, N), *fr = out(c, R, TMHIP_FIELD_EO);
  CK(tmhip_assign_to_64(c, fr, fs, N));
  done(c, R);
}

// ------------------------------------------------------------------ solver
/* solver/cg_her.c:62-141.  For the e/o operators of this library the whole solve runs
 * device-resident (tmhip_cg_her); for any other `f` the reference loop is executed with the
 * drop-in linalg in COHERENT mode, which is correct for an arbitrary host-side f (cg_her_generic, at the end of this file). */
int cg_her(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N,
           matrix_mult f) {
  const int op = dev_op_of(f, N, TMHIP_S_CG);
  if (op < 0) return cg_her_generic(P, Q, max_iter, eps_sq, rel_prec, N, f);
  tmhip_ctx *c = ses.refresh_for(op);
  tmhip_field *fq = in(c, Q, TMHIP_FIELD_EO), *fp = in(c, P, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_cg_her(c, fp, fq, max_iter, eps_sq, rel_prec, N, op, &iters, nullptr, 0));
  done(c, P);          // coherent mode: the solution is on the host when we return; resident mode: after tmlqcd_hip_sync_to_host
  return iters;
}

/* solver/bicgstab_complex.c:49-116.  For the rows of the operator table that name BiCGstab, on an unsplit lattice, the whole solve
 * runs device-resident (tmhip_bicgstab_complex); for any other f the reference's loop runs over the drop-in linalg in coherent mode (bicgstab_complex_generic). */
int bicgstab_complex(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N, matrix_mult f) {
  const int op = dev_op_of(f, N, TMHIP_S_BICG);
  if (op < 0 || g_nproc_t > 1) return bicgstab_complex_generic(P, Q, max_iter, eps_sq, rel_prec, N, f);
  tmhip_ctx *c = ses.refresh_for(op);
  const int kind = op_kind(op);
  tmhip_field *fq = in(c, Q, kind), *fp = in(c, P, kind);
  int iters = -1;
  CK(tmhip_bicgstab_complex(c, fp, fq, max_iter, eps_sq, rel_prec, N, op, &iters, nullptr, 0));
  done(c, P);
  return iters;
}

/* solver/chrono_guess.c:82-172.  The stored solutions, trial and phi are ordinary mirrors; the orthogonalisation changes the stored
 * vectors older than the newest one, so those are handed back as written. */
int chrono_guess(spinor *const trial, spinor *const phi, spinor **const v, int index_array[], const int _N, const int _n, const int V,
                 matrix_mult f) {
  if (_N > 20) die("chrono_guess: a list of more than 20 vectors is not supported (the reference's buffers hold max_N = 20)");
  if (_N <= 0 || _n <= 0) {   /* :168, and the empty list */
    if (V > 0) lin_op(V, wr(trial), none(), none(), [&](Ctx c, Fld ft, Fld, Fld, int) { CK(tmhip_field_zero(c, ft)); });
    return 0;
  }
  if (_n > _N) die("chrono_guess: more vectors than the list holds");
  const int op = dev_op_of(f, V, TMHIP_S_CG);
  if (op < 0) return chrono_guess_generic(trial, phi, v, index_array, _n, V, f);
  tmhip_ctx *c = ses.refresh_for(op);
  tmhip_field *fv[20];
  for (int i = 0; i < _n; i++) fv[i] = in(c, v[index_array[i]], TMHIP_FIELD_EO);
  tmhip_field *fphi = in(c, phi, TMHIP_FIELD_EO), *ft = out(c, trial, TMHIP_FIELD_EO);
  CK(tmhip_chrono_guess(c, ft, fphi, fv, _n, op, V, nullptr, nullptr));
  for (int i = 0; i < _n - 1; i++) done(c, v[index_array[i]]);
  done(c, trial);
  return 0;
}
/* solver/chrono_guess.c:43-75 */
void chrono_add_solution(spinor *const trial, spinor **const v, int index_array[], const int _N, int *_n, const int V) {
  if (_N <= 0) return;
  if (*_n < _N) {
    index_array[*_n] = *_n;
    *_n += 1;
  } else {
    for (int i = 1; i < _N; i++) index_array[i - 1] = index_array[i];   /* the oldest slot is written next */
    index_array[_N - 1] = _N > 1 ? (index_array[_N - 2] + 1) % _N : 0;   /* (a list of one vector: the reference reads index_array[-1], and anything % 1 is 0) */
  }
  const int slot = index_array[(*_n < _N ? *_n : _N) - 1];
  const double norm = sqrt(square_norm(trial, V, 1));
  mul_r(v[slot], 1 / norm, trial, V);
}

/* solver/mixed_cg_her.c:65-202 with f = Qtm_pm_psi: fp32 inner CG + fp64 defect correction, all in HBM */
static_assert(sizeof(tmlqcd_solver_params) == 144 && offsetof(tmlqcd_solver_params, mcg_delta) == 52,
              "solver_params_t layout (solver/solver_params.h:46-109)");
/* solver/cg_her_nd.c:57-160 with f = Qtm_pm_ndpsi or Qsw_pm_ndpsi, device-resident */
int cg_her_nd(spinor *const P_up, spinor *P_dn, spinor *const Q_up, spinor *const Q_dn, const int max_iter, double eps_sq,
              const int rel_prec, const int N, matrix_mult_nd f) {
  const int op = dev_nd_op_of(f, N);
  if (op < 0) die("cg_her_nd: only f = Qtm_pm_ndpsi / Qsw_pm_ndpsi on VOLUME/2 sites runs on the device");
  tmhip_ctx *c = ses.refresh_nd("cg_her_nd");
  tmhip_field *fqu = in(c, Q_up, TMHIP_FIELD_EO), *fqd = in(c, Q_dn, TMHIP_FIELD_EO);
  tmhip_field *fpu = in(c, P_up, TMHIP_FIELD_EO), *fpd = in(c, P_dn, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_cg_her_nd_op(c, fpu, fpd, fqu, fqd, max_iter, eps_sq, rel_prec, N, op, &iters));
  done(c, P_up); done(c, P_dn);
  return iters;
}
/* solver/cg_mms_tm_nd.c:64-215 with M_ndpsi = Qtm_pm_ndpsi or Qsw_pm_ndpsi, device-resident */
int cg_mms_tm_nd(spinor **const Pup, spinor **const Pdn, spinor *const Qup, spinor *const Qdn, tmlqcd_solver_params *sp) {
  const int op = dev_nd_op_of(sp->M_ndpsi, sp->sdim);
  if (op < 0) die("cg_mms_tm_nd: only M_ndpsi = Qtm_pm_ndpsi / Qsw_pm_ndpsi on VOLUME/2 sites runs on the device");
  const int n = sp->no_shifts;
  if (n < 1 || n > 32) die("cg_mms_tm_nd: no_shifts must be in [1, 32]");
  tmhip_ctx *c = ses.refresh_nd("cg_mms_tm_nd");
  tmhip_field *fqu = in(c, Qup, TMHIP_FIELD_EO), *fqd = in(c, Qdn, TMHIP_FIELD_EO);
  tmhip_field *fu[32], *fd[32];
  for (int s = 0; s < n; s++) { fu[s] = out(c, Pup[s], TMHIP_FIELD_EO); fd[s] = out(c, Pdn[s], TMHIP_FIELD_EO); }
  int iters = -1;
  CK(tmhip_cg_mms_tm_nd_op(c, fu, fd, fqu, fqd, sp->shifts, n, sp->max_iter, sp->squared_solver_prec, sp->rel_prec, op, &iters));
  for (int s = 0; s < n; s++) { done(c, Pup[s]); done(c, Pdn[s]); }
  return iters;
}

/* solver/cg_mms_tm.c:65-197; whatever does not run on the device goes through the reference loop (cg_mms_tm_generic, at the end of this file) */
int cg_mms_tm(spinor **const P, spinor *const Q, tmlqcd_solver_params *sp, double *cgmms_reached_prec) {
  const int N = sp->sdim, n = sp->no_shifts, max_iter = sp->max_iter, rel_prec = sp->rel_prec;
  const double eps_sq = sp->squared_solver_prec;
  const int op = dev_op_of(sp->M_psi, N, TMHIP_S_MMS);
  int iters = -1;
  if (op >= 0 && g_nproc_t == 1 && n >= 1 && n <= 32 && max_iter >= 1) {
    tmhip_ctx *c = ses.refresh_for(op);
    const int kind = op_kind(op);
    tmhip_field *fq = in(c, Q, kind), *fp[32];
    for (int s = 0; s < n; s++) fp[s] = out(c, P[s], kind);
    double reached = 0.0;
    CK(tmhip_cg_mms_tm(c, fp, fq, sp->shifts, n, max_iter, eps_sq, rel_prec, N, op, &iters, &reached));
    for (int s = 0; s < n; s++) done(c, P[s]);
    *cgmms_reached_prec = reached;
  } else {
    iters = cg_mms_tm_generic(P, Q, sp, cgmms_reached_prec);
  }
  if (&g_sloppy_precision) g_sloppy_precision = 0;   /* :192 */
  return iters;
}

int mixed_cg_her(spinor *const P, spinor *const Q, tmlqcd_solver_params, const int max_iter, double eps_sq,
                 const int rel_prec, const int N, matrix_mult f, matrix_mult32) {
  const int op = dev_op_of(f, N, TMHIP_S_MIXED);
  if (op < 0) die("mixed_cg_her: only f = Qtm_pm_psi / Qsw_pm_psi on VOLUME/2 sites runs on the device");
  const double innereps = &mixcg_innereps ? mixcg_innereps : 5.0e-5;           /* default_input_values.h:193 */
  const int max_inner = &mixcg_maxinnersolverit ? mixcg_maxinnersolverit : 5000; /* default_input_values.h:194 */
  tmhip_ctx *c = ses.refresh_for(op);
  int iters = -1, outer = 0;
  apply(c, TMHIP_FIELD_EO, P, Q, nullptr, [&](Ctx, Fld fp, Fld fq, Fld) {
    CK(tmhip_mixed_cg_her(c, fp, fq, max_iter, eps_sq, rel_prec, N, op, innereps, max_inner, &iters, &outer));
  });
  return iters;
}

/* solver/rg_mixed_cg_her.c:180-347 with (f, f32) = (Qtm_pm_psi, Qtm_pm_psi_32) or (Qsw_pm_psi, Qsw_pm_psi_32) */
int rg_mixed_cg_her(spinor *const P, spinor *const Q, tmlqcd_solver_params solver_params, const int max_iter,
                    const double eps_sq, const int rel_prec, const int N, matrix_mult f, matrix_mult32) {
  const int op = dev_op_of(f, N, TMHIP_S_MIXED);
  if (op < 0) die("rg_mixed_cg_her: only f = Qtm_pm_psi / Qsw_pm_psi on VOLUME/2 sites runs on the device");
  tmhip_ctx *c = ses.refresh_for(op);
  int iters = -1;
  apply(c, TMHIP_FIELD_EO, P, Q, nullptr, [&](Ctx, Fld fp, Fld fq, Fld) {
    CK(tmhip_rg_mixed_cg_her(c, fp, fq, max_iter, eps_sq, rel_prec, N, op, solver_params.mcg_delta, &iters, nullptr, nullptr, nullptr));
  });
  return iters;
}

/* solver/rg_mixed_cg_her_nd.c:189-341 with (f, f32) = (Qtm_pm_ndpsi, Qtm_pm_ndpsi_32), device-resident; residency as cg_her_nd */
int rg_mixed_cg_her_nd(spinor *const P_up, spinor *const P_dn, spinor *const Q_up, spinor *const Q_dn, tmlqcd_solver_params solver_params,
                       const int max_iter, const double eps_sq, const int rel_prec, const int N, matrix_mult_nd f, matrix_mult_nd32) {
  const int op = dev_nd_op_of(f, N);
  if (op < 0 || !tmhip_op_taken(tmhip_nd_op_row_of(op), TMHIP_S_MIXED)) die("rg_mixed_cg_her_nd: only f = Qtm_pm_ndpsi on VOLUME/2 sites runs on the device");
  tmhip_ctx *c = ses.refresh_nd("rg_mixed_cg_her_nd");
  tmhip_field *fqu = in(c, Q_up, TMHIP_FIELD_EO), *fqd = in(c, Q_dn, TMHIP_FIELD_EO);
  tmhip_field *fpu = out(c, P_up, TMHIP_FIELD_EO), *fpd = out(c, P_dn, TMHIP_FIELD_EO);   /* zero start: P is written only */
  int iters = -1;
  CK(tmhip_rg_mixed_cg_her_nd(c, fpu, fpd, fqu, fqd, max_iter, eps_sq, rel_prec, N, op, solver_params.mcg_delta, &iters, nullptr, nullptr, nullptr));
  done(c, P_up); done(c, P_dn);
  return iters;
}

/* solver/mixed_cg_mms_tm_nd.c:69-511 with (M_ndpsi, M_ndpsi32) = (Qtm_pm_ndpsi, Qtm_pm_ndpsi_32), device-resident; residency as cg_mms_tm_nd */
int mixed_cg_mms_tm_nd(spinor **const Pup, spinor **const Pdn, spinor *const Qup, spinor *const Qdn, tmlqcd_solver_params *sp) {
  const int op = dev_nd_op_of(sp->M_ndpsi, sp->sdim);
  if (op < 0 || !tmhip_op_taken(tmhip_nd_op_row_of(op), TMHIP_S_MIXED) || (void *)sp->M_ndpsi32 != (void *)&Qtm_pm_ndpsi_32)
    die("mixed_cg_mms_tm_nd: only M_ndpsi = Qtm_pm_ndpsi with M_ndpsi32 = Qtm_pm_ndpsi_32 on VOLUME/2 sites runs on the device");
  const int n = sp->no_shifts;
  if (n < 1 || n > 32) die("mixed_cg_mms_tm_nd: no_shifts must be in [1, 32]");
  tmhip_ctx *c = ses.refresh_nd("mixed_cg_mms_tm_nd");
  tmhip_field *fqu = in(c, Qup, TMHIP_FIELD_EO), *fqd = in(c, Qdn, TMHIP_FIELD_EO);
  tmhip_field *fu[32], *fd[32];
  for (int s = 0; s < n; s++) { fu[s] = out(c, Pup[s], TMHIP_FIELD_EO); fd[s] = out(c, Pdn[s], TMHIP_FIELD_EO); }
  int iters = -1;
  CK(tmhip_mixed_cg_mms_tm_nd(c, fu, fd, fqu, fqd, sp->shifts, n, sp->max_iter, sp->squared_solver_prec, sp->rel_prec, op, &iters, nullptr, nullptr));
  for (int s = 0; s < n; s++) { done(c, Pup[s]); done(c, Pdn[s]); }
  return iters;
}

// ------------------------------------------------------------------ fermion force
/* deriv_Sb.c:401-700 */
void deriv_Sb(const int ieo, spinor *const l, spinor *const k, hamiltonian_field_t *const hf, const double factor) {
  tmhip_ctx *c = ses.refresh(true);
  tmhip_field *fl = in(c, l, TMHIP_FIELD_EO), *fk = in(c, k, TMHIP_FIELD_EO);
  force_begin(c);
  CK(tmhip_deriv_Sb(c, ieo, fl, fk, factor));
  force_end(hf);
}
/* Clover part of the force under helper names (the reference keeps sw_deriv_nd / sw_spinor in the same objects, which therefore
 * stay on the link line): the statements of cloverdet_derivative, monomial/cloverdet_monomial.c:67-72,125-147 */
void tmlqcd_hip_swpm_zero(void) { CK(tmhip_swpm_zero(ses.refresh(false))); }
void tmlqcd_hip_sw_spinor_eo(const int ieo, const spinor *const kk, const spinor *const ll, const double fac) {   /* clover_deriv.c:252 */
  tmhip_ctx *c = ses.refresh(false);
  tmhip_field *fk = in(c, kk, TMHIP_FIELD_EO), *fl = in(c, ll, TMHIP_FIELD_EO);
  CK(tmhip_sw_spinor_eo(c, ieo, fk, fl, fac));
}
void tmlqcd_hip_sw_deriv(const int ieo, const double mu) {   /* clover_deriv.c:72 */
  tmhip_ctx *c = ses.refresh_clover();
  CK(tmhip_sw_deriv(c, ieo, mu));
}
void tmlqcd_hip_sw_all(hamiltonian_field_t *const hf, const double kappa, const double c_sw) {   /* clover_accumulate_deriv.c:58 */
  tmhip_ctx *c = ses.refresh(true);
  force_begin(c);
  CK(tmhip_sw_all(c, &hf->gaugefield[0][0], kappa, c_sw));
  force_end(hf);
}
void tmlqcd_hip_flush_derivative(hamiltonian_field_t *const hf) {
  if (!ses.deriv_pending) return;
  CK(tmhip_derivative_download(ctx(), &hf->derivative[0][0], 1));
  ses.deriv_pending = false;
}

// ------------------------------------------------------------------ gauge monomial
/* measure_gauge_action.c:46-189, measure_rectangles.c:51-140 on the device links: gf must be the field this library mirrors
 * (g_gauge_field, which hf->gaugefield points to); it goes up by the rules of every other entry point (refresh), and in resident mode
 * the device's own, newer links are the ones measured.  T-split ranks: the three measures return the sum over all ranks, the same
 * bits on every rank, as the reference does after its MPI_Allreduce (the core entry points return the rank's share unless told so);
 * measure_rectangles and a rectangle force end the program there (the device holds a one-deep link halo). */
static tmhip_ctx *gauge_links(const su3 **const gf, const char *who) {
  if (!gf || &gf[0][0] != &g_gauge_field[0][0]) die(who);
  tmhip_ctx *c = ses.refresh(true);
  CK(tmhip_set_option(c, "gauge_global_sums", 1));
  return c;
}
double measure_plaquette(const su3 **const gf) {
  tmhip_ctx *c = gauge_links(gf, "measure_plaquette: gf is not g_gauge_field");
  double r = 0.0;
  CK(tmhip_measure_plaquette(c, &r));
  return r;
}
double measure_gauge_action(const su3 **const gf, const double lambda) {
  tmhip_ctx *c = gauge_links(gf, "measure_gauge_action: gf is not g_gauge_field");
  double r = 0.0;
  CK(tmhip_measure_gauge_action(c, lambda, &r));
  GaugeInfo.plaquetteEnergy = r;                                  /* measure_gauge_action.c:187 */
  return r;
}
double measure_rectangles(const su3 **const gf) {
  tmhip_ctx *c = gauge_links(gf, "measure_rectangles: gf is not g_gauge_field");
  double r = 0.0;
  CK(tmhip_measure_rectangles(c, &r));
  return r;
}
/* gauge_derivative / gauge_EMderivative (monomial/gauge_monomial.c:48-162) with the monomial's parameters as arguments; accumulates
 * like tmlqcd_hip_sw_all: into hf->derivative before returning (coherent), or held on the device until tmlqcd_hip_flush_derivative /
 * tmlqcd_hip_update_momenta (resident) */
void tmlqcd_hip_gauge_derivative(hamiltonian_field_t *const hf, const double beta, const double c0, const double c1, const int use_rectangles,
                                 const double glambda) {
  tmhip_ctx *c = gauge_links((const su3 **)hf->gaugefield, "tmlqcd_hip_gauge_derivative: hf->gaugefield is not g_gauge_field");
  force_begin(c);
  CK(tmhip_gauge_derivative(c, beta, c0, c1, use_rectangles, glambda));
  force_end(hf);
}

// ------------------------------------------------------------------ gradient flow and field strength (flow.hip)
/* meas/measure_clover_field_strength_observables.c:55-225 on the device links, by the rules of the gauge measures above.  Unsplit
 * lattices: on a T-split rank the core entry point refuses and the program ends with its message, as for the rectangle measures. */
void measure_clover_field_strength_observables(const su3 **const gf, field_strength_obs_t *const fso) {
  tmhip_ctx *c = gauge_links(gf, "measure_clover_field_strength_observables: gf is not g_gauge_field");
  CK(tmhip_measure_field_strength(c, &fso->E, &fso->Q));
}
/* gradient_flow_measurement (meas/gradient_flow.c:132-239) with gf_eps / gf_tmax of measurement_list[id] as arguments: the flow runs on
 * device copies of the links (g_gauge_field and the device's resident links are not modified), one line per pair of steps goes to
 * gradflow.<traj> in the working directory, flushed as the reference does. */
void tmlqcd_hip_gradient_flow_measurement(const int traj, const double eps, const double tmax) {
  tmhip_ctx *c = gauge_links((const su3 **)g_gauge_field, "tmlqcd_hip_gradient_flow_measurement: no g_gauge_field");
  if (g_nproc_t > 1) die("tmlqcd_hip_gradient_flow_measurement: not available on T-split ranks (the link halo would need a refresh after every stage)");
  char filename[100];
  snprintf(filename, 100, "gradflow.%06d", traj);
  FILE *outfile = fopen(filename, "w");
  if (outfile == NULL) {
    char error_message[200];
    snprintf(error_message, 200, "Couldn't open %s for writing during gradient flow measurement!", filename);
    die(error_message);
  }
  fprintf(outfile, "traj t P Eplaq Esym tsqEplaq tsqEsym Wsym Qsym\n");
  // the loop of gradient_flow.c:172-222 on the step-wise entry points, so that every line is on disk when its pair of steps is done
  double t[3] = {0.0, 0.0, 0.0}, P[3] = {0.0, 0.0, 0.0}, E[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0};
  CK(tmhip_flow_begin(c));
  CK(tmhip_flow_observables(c, &P[2], &E[2], &Q[2]));
  while (t[1] < tmax) {
    t[0] = t[2]; E[0] = E[2]; Q[0] = Q[2]; P[0] = P[2];
    for (int step = 1; step < 3; ++step) {
      t[step] = t[step - 1] + eps;
      CK(tmhip_flow_step(c, eps));
      CK(tmhip_flow_observables(c, &P[step], &E[step], &Q[step]));
    }
    const double W = t[1] * t[1] * (2 * E[1] + t[1] * ((E[2] - E[0]) / (2 * eps)));
    const double tsqE = t[1] * t[1] * E[1];
    fprintf(outfile, "%06d %f %2.12lf %2.12lf %2.12lf %2.12lf %2.12lf %2.12lf %.12lf \n", traj, t[1], P[1], 36 * (1 - P[1]), E[1],
            t[1] * t[1] * 36 * (1 - P[1]), tsqE, W, Q[1]);
    fflush(outfile);
  }
  CK(tmhip_flow_end(c));
  fclose(outfile);
}

// ------------------------------------------------------------------ the other online measurements (meas.hip)
/* The site loops of correlators_measurement (meas/correlators.c:154-170, dir 0) and pion_norm_measurement (meas/pion_norm.c:93-107,
 * dir 3) on the two e/o halves of the propagator, which are inputs like any other (uploaded unless their mirrors are current).  The
 * raw sums of this rank: the reference's MPI_Reduce, normalisation and files stay the caller's. */
void tmlqcd_hip_slice_correlators(const spinor *const even, const spinor *const odd, const int dir, double *const pp, double *const pa, double *const p4) {
  tmhip_ctx *c = ses.refresh(false);
  tmhip_field *fe = in(c, even, TMHIP_FIELD_EO), *fo = in(c, odd, TMHIP_FIELD_EO);
  CK(tmhip_slice_correlators(c, fe, fo, dir, pp, pa, p4));
}
static tmhip_ctx *unsplit_gauge_links(const su3 **const gf, const char *who, const char *split) {
  if (g_nproc_t > 1) die(split);
  return gauge_links(gf, who);
}
/* meas/oriented_plaquettes.c:39-86 on the device links, by the rules of the gauge measures above */
void measure_oriented_plaquettes(const su3 **const gf, double *plaq) {
  tmhip_ctx *c = unsplit_gauge_links(gf, "measure_oriented_plaquettes: gf is not g_gauge_field", "measure_oriented_plaquettes: not available on T-split ranks");
  CK(tmhip_measure_oriented_plaquettes(c, plaq));
}
/* meas/oriented_plaquettes.c:88-112; neither function reads measurement_list */
void oriented_plaquettes_measurement(const int traj, const int id, const int ieo) {
  (void)ieo;
  double plaq[6];
  measure_oriented_plaquettes((const su3 **)g_gauge_field, plaq);
  char filename[] = "oriented_plaquettes.data";
  FILE *outfile = fopen(filename, "a");
  if (outfile == NULL) {
    char error_message[200];
    snprintf(error_message, 200, "Couldn't open %s for appending during measurement %d!", filename, id);
    die(error_message);
  }
  fprintf(outfile, "%.8d %14.12lf %14.12lf %14.12lf %14.12lf %14.12lf %14.12lf\n", traj, plaq[0], plaq[1], plaq[2], plaq[3], plaq[4], plaq[5]);
  fclose(outfile);
}
/* The Polyakov loop along any direction on the device links: polyakov_loop (meas/polyakov_loop.c:51-157) for dir 2 and 3, the value
 * polyakov_loop_dir (:325-558) writes for dir 0 and 3 */
void tmlqcd_hip_polyakov_loop(double pl[2], const int dir) {
  tmhip_ctx *c = unsplit_gauge_links((const su3 **)g_gauge_field, "tmlqcd_hip_polyakov_loop: no g_gauge_field", "tmlqcd_hip_polyakov_loop: not available on T-split ranks");
  CK(tmhip_polyakov_loop(c, dir, &pl[0], &pl[1]));
}
int tmlqcd_hip_polyakov_loop_dir(const int nstore, const int dir) {
  if (dir != 0 && dir != 3) {
    fprintf(stderr, "Wrong direction; must be 0 (t) or 3 (z)\n");
    return -1;
  }
  double pl[2];
  tmlqcd_hip_polyakov_loop(pl, dir);
  char filename[50];
  snprintf(filename, 50, "polyakovloop_dir%1d", dir);
  FILE *ofs = fopen(filename, nstore == 0 ? "w" : "a");
  if (ofs == NULL) {
    fprintf(stderr, "Could not open file %s for writing\n", filename);
    return -1;
  }
  fprintf(ofs, "%4d\t%2d\t%25.16e\t%25.16e\n", nstore, dir, pl[0], pl[1]);
  fclose(ofs);
  return 0;
}

// ------------------------------------------------------------------ LapH: the 3D Laplacian and its eigensystem (laph.hip)
// two colour-vector fields of the session's context for the host vectors of Jacobi; made again when the context is
static tmhip_cvfield *laph_io[2] = {nullptr, nullptr};
static tmhip_ctx *laph_io_ctx = nullptr;
static void laph_fields(tmhip_ctx *c) {
  if (laph_io_ctx == c && laph_io[0]) return;
  for (int i = 0; i < 2; i++) { tmhip_cvfield_free(c, laph_io[i]); laph_io[i] = nullptr; }
  for (int i = 0; i < 2; i++) CK(tmhip_cvfield_alloc(c, &laph_io[i]));
  laph_io_ctx = c;
}
/* jacobi.c:43-72 without its MPI exchange: l and k are host vectors of SPACEVOLUME sites, copied in and out */
void Jacobi(su3_vector *const l, su3_vector *const k, int t) {
  tmhip_ctx *c = unsplit_gauge_links((const su3 **)g_gauge_field, "Jacobi: no g_gauge_field", "Jacobi: not available on T-split ranks");
  if (!l || !k || l == k) die("Jacobi: l and k must be two vectors");
  if (t < 0 || t >= T) die("Jacobi: t is outside [0, T)");
  laph_fields(c);
  CK(tmhip_cvfield_upload_slices(c, laph_io[0], k, t, 1));
  CK(tmhip_laph_apply(c, laph_io[1], laph_io[0], t, 1));
  CK(tmhip_cvfield_download_slices(c, laph_io[1], l, t, 1));
}
/* the loop over the time-slices of eigenvalues_Jacobi.c:120-209 for all of them at once: the nev lowest eigenpairs of every slice and
 * the files of its branch without MPI in the working directory; returns the number of slices with all nev pairs converged */
int tmlqcd_hip_laph_eigensystem(const int nev, const double prec, const int max_apps, const int nstore) {
  tmhip_ctx *c = unsplit_gauge_links((const su3 **)g_gauge_field, "tmlqcd_hip_laph_eigensystem: no g_gauge_field", "tmlqcd_hip_laph_eigensystem: not available on T-split ranks");
  if (nev < 1 || nev > TMHIP_LAPH_MAX_BASIS - 2) die("tmlqcd_hip_laph_eigensystem: the number of eigenpairs must be in [1, 126]");
  std::vector<tmhip_cvfield *> ev(nev, nullptr);
  for (int i = 0; i < nev; i++) CK(tmhip_cvfield_alloc(c, &ev[i]));
  std::vector<double> evals((size_t)T * nev), resid((size_t)T * nev);
  std::vector<int> conv(T), apps(T);
  int done_slices = 0;
  for (int t0 = 0; t0 < T; t0 += 256) {   // a call of the library takes 256 slices
    const int nt = T - t0 < 256 ? T - t0 : 256;
    CK(tmhip_laph_eigensystem(c, t0, nt, nev, prec, max_apps, ev.data(), evals.data() + (size_t)t0 * nev, resid.data() + (size_t)t0 * nev, conv.data() + t0, apps.data() + t0));
    CK(tmhip_laph_write(c, ".", nstore, t0, nt, nev, ev.data(), evals.data() + (size_t)t0 * nev));
  }
  for (int t = 0; t < T; t++) done_slices += conv[t] == nev;
  for (int i = 0; i < nev; i++) tmhip_cvfield_free(c, ev[i]);
  return done_slices;
}

// ------------------------------------------------------------------ polynomial monomial NDPOLY (poly.hip)
/* linalg/assign_mul_add_mul_add_mul_add_mul_r.c: R = c1 R + c2 S + c3 U + c4 V, N = VOLUME/2 (the only length its callers use) */
void assign_mul_add_mul_add_mul_add_mul_r(spinor *const R, spinor *const S, spinor *const U, spinor *const V, const double c1, const double c2,
                                          const double c3, const double c4, const int N) {
  tmhip_ctx *c = ses.refresh(false);
  if (N == 0) return;
  if (N != VOLUME / 2) die("assign_mul_add_mul_add_mul_add_mul_r: N must be VOLUME/2");
  tmhip_field *fs = in(c, S, TMHIP_FIELD_EO), *fu = in(c, U, TMHIP_FIELD_EO), *fv = in(c, V, TMHIP_FIELD_EO), *fr = in(c, R, TMHIP_FIELD_EO);
  CK(tmhip_assign_mul_add_mul_add_mul_add_mul_r(c, fr, fs, fu, fv, c1, c2, c3, c4));
  done(c, R);
}
/* Ptilde_nd.c:102-203 with Qsq = Qtm_pm_ndpsi or Qsw_pm_ndpsi; the interval is phmc_cheb_evmin / phmc_cheb_evmax at call time */
void Ptilde_ndpsi(spinor *R_s, spinor *R_c, double *dd, int n, spinor *S_s, spinor *S_c, matrix_mult_nd Qsq) {
  const int op = dev_nd_op_of(Qsq, VOLUME / 2);
  if (op < 0) die("Ptilde_ndpsi: only Qsq = Qtm_pm_ndpsi / Qsw_pm_ndpsi runs on the device");
  if (!&phmc_cheb_evmin || !&phmc_cheb_evmax) die("Ptilde_ndpsi: the host program has no phmc_cheb_evmin / phmc_cheb_evmax");
  const double evmin = phmc_cheb_evmin, evmax = phmc_cheb_evmax;
  apply2(ses.refresh_nd("Ptilde_ndpsi"), R_s, R_c, S_s, S_c, [&](Ctx c, Fld frs, Fld frc, Fld fss, Fld fsc) {
    CK(tmhip_Ptilde_ndpsi(c, frs, frc, dd, n, fss, fsc, evmin, evmax, op));
  });
}
// the three bodies run with g_mubar / g_epsbar of the host (ndpoly_set_global_parameter has set them) and phmc_invmaxev = the monomial's EVMaxInv
static tmhip_ctx *ndpoly_refresh(const char *who, const double EVMaxInv) {
  if (&phmc_exact_poly && phmc_exact_poly == 1) {
    char m[160];
    snprintf(m, sizeof(m), "%s: the phmc_exact_poly == 1 branches are not built", who);
    die(m);
  }
  tmhip_ctx *c = ses.refresh_nd(who);
  CK(tmhip_set_nd(c, &g_mubar ? g_mubar : 0., &g_epsbar ? g_epsbar : 0., EVMaxInv));
  return c;
}
/* ndpoly_monomial.c:69-117; Cpol = sqrt(MDPolyLocNormConst) (:552) */
int tmlqcd_hip_ndpoly_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots,
                                 const int MDPolyDegree, const double MDPolyLocNormConst, const double EVMaxInv) {
  tmhip_ctx *c = ndpoly_refresh("tmlqcd_hip_ndpoly_derivative", EVMaxInv);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  force_begin(c);
  CK(tmhip_ndpoly_derivative(c, fu, fd, (const double *)MDPolyRoots, MDPolyDegree, sqrt(MDPolyLocNormConst), EVMaxInv));
  force_end(hf);
  return 0;
}
/* ndpoly_monomial.c:179-209, 255-256 on the Gaussian field the caller has drawn into pf / pf2; phmc_cheb_evmax = 1 (:561) */
int tmlqcd_hip_ndpoly_heatbath(spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots, const int MDPolyDegree,
                               const double MDPolyLocNormConst, const double EVMaxInv, const double *PtildeCoefs, const int PtildeDegree,
                               const double EVMin, double *energy0) {
  tmhip_ctx *c = ndpoly_refresh("tmlqcd_hip_ndpoly_heatbath", EVMaxInv);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  CK(tmhip_ndpoly_heatbath(c, fu, fd, (const double *)MDPolyRoots, MDPolyDegree, sqrt(MDPolyLocNormConst), EVMaxInv, PtildeCoefs, PtildeDegree, EVMin, 1.0,
                           energy0));
  done(c, pf); done(c, pf2);
  return 0;
}
/* ndpoly_monomial.c:282-368; returns the number of correction steps taken */
int tmlqcd_hip_ndpoly_acc(spinor *const pf, spinor *const pf2, const _Complex double *MDPolyRoots, const int MDPolyDegree, const double MDPolyLocNormConst,
                          const double EVMaxInv, const double *MDPolyCoefs, const double *PtildeCoefs, const int PtildeDegree, const double EVMin,
                          const double PrecisionHfinal, double *energy1) {
  tmhip_ctx *c = ndpoly_refresh("tmlqcd_hip_ndpoly_acc", EVMaxInv);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  int corrections = 0;
  CK(tmhip_ndpoly_acc(c, fu, fd, (const double *)MDPolyRoots, MDPolyDegree, sqrt(MDPolyLocNormConst), EVMaxInv, MDPolyCoefs, PtildeCoefs, PtildeDegree, EVMin,
                      1.0, PrecisionHfinal, energy1, &corrections, nullptr));
  return corrections;
}

// ------------------------------------------------------------------ eigenvalue measurement (eig.hip)
// max_iterations bounds the restarts: the run takes at most that many Lanczos cycles (option "eig_restarts", put back to "no bound" after
// the call); the operator applications themselves are not capped
static const int EIG_NO_APP_CAP = 2000000000;
extern "C++" {
template <class F> inline void with_restarts(tmhip_ctx *c, const int max_iterations, F body) {
  CK(tmhip_set_option(c, "eig_restarts", max_iterations < 1 ? 1 : max_iterations));
  body();
  CK(tmhip_set_option(c, "eig_restarts", 0));
}
}
/* solver/eigenvalues_bi.c:59-152 with Qsq = Qtm_pm_ndbipsi or Qsw_pm_ndbipsi, which are known here by their addresses only */
double eigenvalues_bi(int *nev, const int max_iterations, const double prec, const int maxmin, matrix_mult_bi Qsq) {
  int op = -1;
  if (Qsq && Qsq == &Qtm_pm_ndbipsi) op = TMHIP_ND_OP_QTM_PM;
  else if (Qsq && Qsq == &Qsw_pm_ndbipsi) op = TMHIP_ND_OP_QSW_PM;
  if (op < 0) die("eigenvalues_bi: only Qsq = Qtm_pm_ndbipsi / Qsw_pm_ndbipsi runs on the device");
  if (!nev || *nev < 1 || *nev > 62) die("eigenvalues_bi: the number of eigenvalues must be in [1, 62]");
  tmhip_ctx *c = ses.refresh_nd("eigenvalues_bi");
  double evals[64], resid[64];
  int converged = 0, apps = 0;
  with_restarts(c, max_iterations, [&] {
    CK(tmhip_eigenvalues_nd(c, op, *nev, maxmin ? 1 : 0, prec < 1.e-14 ? 1.e-14 : prec, EIG_NO_APP_CAP, nullptr, nullptr, evals, resid, &converged, &apps));
  });
  *nev = converged;
  return evals[0];
}
/* phmc.c:205-253 */
int tmlqcd_hip_phmc_compute_ev(const int trajectory_counter, const int id, const char *name, const double EVMin, const int clover, const double prec,
                               double *ev_min, double *ev_max) {
  tmhip_ctx *c = ses.refresh_nd("tmlqcd_hip_phmc_compute_ev");
  const int op = clover ? TMHIP_ND_OP_QSW_PM : TMHIP_ND_OP_QTM_PM;
  double ev[2] = {0., 0.}, resid = 0.;
  for (int maxmin = 0; maxmin < 2; maxmin++) {
    int converged = 0, apps = 0;
    with_restarts(c, 1000, [&] {   /* max_iter_ev = 1000, :218 */
      CK(tmhip_eigenvalues_nd(c, op, 1, maxmin, prec < 1.e-14 ? 1.e-14 : prec, EIG_NO_APP_CAP, nullptr, nullptr, &ev[maxmin], &resid, &converged, &apps));
    });
  }
  const char *mname = name ? name : "";
  if (ev[1] > 1.) fprintf(stderr, "\nWarning: largest eigenvalue for monomial %s larger than upper bound!\n\n", mname);
  if (ev[0] < EVMin) fprintf(stderr, "\nWarning: smallest eigenvalue for monomial %s smaller than lower bound!\n\n", mname);
  char filename[100];
  snprintf(filename, sizeof(filename), "monomial-%.2d.data", id);
  FILE *countfile = fopen(filename, "a");
  if (!countfile) die("tmlqcd_hip_phmc_compute_ev: cannot open the monomial's data file for appending");
  fprintf(countfile, "%.8d %1.5e %1.5e %1.5e %1.5e\n", trajectory_counter, ev[0], ev[1], EVMin, 1.);
  fclose(countfile);
  if (ev_min) *ev_min = ev[0];
  if (ev_max) *ev_max = ev[1];
  return 0;
}
/* the jdher calls of solver/eigenvalues.c:162-229 */
double tmlqcd_hip_eigenvalues(int *nev, const int max_iterations, const double prec, const int maxmin, spinor *evecs, double *evals) {
  const bool eo = &even_odd_flag ? even_odd_flag != 0 : true;
  const int N = eo ? VOLUME / 2 : VOLUME;
  const int op = dev_op_of(eo ? &Qtm_pm_psi : &Q_pm_psi, N, TMHIP_S_EIG);
  if (op < 0) die("tmlqcd_hip_eigenvalues: Q_pm_psi with a clover term (g_c_sw > 0) does not run on the device");
  if (!nev || !evals || *nev < 1 || *nev > 62) die("tmlqcd_hip_eigenvalues: the number of eigenvalues must be in [1, 62]");
  if (g_nproc_t > 1) die("tmlqcd_hip_eigenvalues: the eigenvalue measurement runs on unsplit lattices only");
  tmhip_ctx *c = ses.refresh_for(op);
  const int kind = op_kind(op), n = *nev;
  const size_t stride = eo ? (size_t)VOLUMEPLUSRAND / 2 : (size_t)VOLUMEPLUSRAND;
  tmhip_field *fv[64];
  if (evecs) for (int i = 0; i < n; i++) fv[i] = in(c, evecs + i * stride, kind);   // evecs[0], when it is not zero, is the start vector
  double resid[64];
  int converged = 0, apps = 0;
  with_restarts(c, max_iterations, [&] {
    CK(tmhip_eigenvalues(c, op, N, n, maxmin ? 1 : 0, prec < 1.e-14 ? 1.e-14 : prec, EIG_NO_APP_CAP, evecs ? fv : nullptr, evals, resid, &converged, &apps));
  });
  if (evecs) for (int i = 0; i < n; i++) done(c, evecs + i * stride);
  *nev = converged;
  return evals[0];
}

// ------------------------------------------------------------------ rational monomials (rational.hip)
/* ndrat_monomial.c:96-160 */
int tmlqcd_hip_ndrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np,
                                const double EVMaxInv, const int max_iter, const double eps_sq, const int rel_prec) {
  tmhip_ctx *c = ses.refresh_nd("tmlqcd_hip_ndrat_derivative");
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  force_begin(c);
  int iters = -1;
  CK(tmhip_ndrat_derivative(c, fu, fd, mu, rmu, np, EVMaxInv, max_iter, eps_sq, rel_prec, &iters));
  force_end(hf);
  return iters;
}
/* ndrat_monomial.c:212-254 */
int tmlqcd_hip_ndrat_heatbath(spinor *const pf, spinor *const pf2, const double *nu, const double *rnu, const int np, const double EVMaxInv,
                              const int max_iter, const double eps_sq, const int rel_prec, double *energy0) {
  return nd_heatbath("tmlqcd_hip_ndrat_heatbath", tmhip_ndrat_heatbath, pf, pf2, nu, rnu, np, EVMaxInv, max_iter, eps_sq, rel_prec, energy0);
}
/* ndrat_monomial.c:281-309 */
int tmlqcd_hip_ndrat_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np, const int max_iter,
                         const double eps_sq, const int rel_prec, double *energy1) {
  return nd_acc("tmlqcd_hip_ndrat_acc", tmhip_ndrat_acc, pf, pf2, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1);
}
/* ndrat_monomial.c:80-184 for type NDCLOVERRAT, after the caller's sw_term + sw_invert_nd (:89-91): swm / swp are zeroed, filled and folded
 * into the derivative on the device (trlog: the monomial's flag, :179-181) */
int tmlqcd_hip_ndcloverrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np,
                                      const double EVMaxInv, const double kappa, const double c_sw, const int trlog, const int max_iter,
                                      const double eps_sq, const int rel_prec) {
  tmhip_ctx *c = ses.refresh_nd("tmlqcd_hip_ndcloverrat_derivative");
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  force_begin(c);
  int iters = -1;
  CK(tmhip_ndcloverrat_derivative(c, fu, fd, mu, rmu, np, EVMaxInv, kappa, c_sw, trlog, max_iter, eps_sq, rel_prec, &iters));
  force_end(hf);
  return iters;
}
int tmlqcd_hip_ndcloverrat_heatbath(spinor *const pf, spinor *const pf2, const double *nu, const double *rnu, const int np, const double EVMaxInv,
                                    const int max_iter, const double eps_sq, const int rel_prec, double *energy0) {
  return nd_heatbath("tmlqcd_hip_ndcloverrat_heatbath", tmhip_ndcloverrat_heatbath, pf, pf2, nu, rnu, np, EVMaxInv, max_iter, eps_sq, rel_prec, energy0);
}
int tmlqcd_hip_ndcloverrat_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const int np, const int max_iter,
                               const double eps_sq, const int rel_prec, double *energy1) {
  return nd_acc("tmlqcd_hip_ndcloverrat_acc", tmhip_ndcloverrat_acc, pf, pf2, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1);
}
/* rat_monomial.c:83-132 (type RAT) */
int tmlqcd_hip_rat_derivative(hamiltonian_field_t *const hf, spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter,
                              const double eps_sq, const int rel_prec) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_rat_derivative");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  force_begin(c);
  int iters = -1;
  CK(tmhip_rat_derivative(c, f, mu, rmu, np, max_iter, eps_sq, rel_prec, &iters));
  force_end(hf);
  return iters;
}
/* rat_monomial.c:175-199 */
int tmlqcd_hip_rat_heatbath(spinor *const pf, const double *nu, const double *rnu, const int np, const int max_iter, const double eps_sq,
                            const int rel_prec, double *energy0) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_rat_heatbath");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_rat_heatbath(c, f, nu, rnu, np, max_iter, eps_sq, rel_prec, energy0, &iters));
  done(c, pf);
  return iters;
}
/* rat_monomial.c:232-250 */
int tmlqcd_hip_rat_acc(spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter, const double eps_sq,
                       const int rel_prec, double *energy1) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_rat_acc");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_rat_acc(c, f, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, &iters));
  return iters;
}
/* rat_monomial.c:66-139 for type CLOVERRAT, after the caller's tmlqcd_hip_sw_term + tmlqcd_hip_sw_invert(EE, 0.) (:76-78): swm / swp are
 * zeroed, filled and folded into the derivative on the device (trlog: the monomial's flag, :134-136) */
int tmlqcd_hip_cloverrat_derivative(hamiltonian_field_t *const hf, spinor *const pf, const double *mu, const double *rmu, const int np, const double kappa,
                                    const double c_sw, const int trlog, const int max_iter, const double eps_sq, const int rel_prec) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_cloverrat_derivative");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  force_begin(c);
  int iters = -1;
  CK(tmhip_cloverrat_derivative(c, f, mu, rmu, np, kappa, c_sw, trlog, max_iter, eps_sq, rel_prec, &iters));
  force_end(hf);
  return iters;
}
/* rat_monomial.c:175-199 on Qsw_pm_psi / Qsw_plus_psi */
int tmlqcd_hip_cloverrat_heatbath(spinor *const pf, const double *nu, const double *rnu, const int np, const int max_iter, const double eps_sq,
                                  const int rel_prec, double *energy0) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_cloverrat_heatbath");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_cloverrat_heatbath(c, f, nu, rnu, np, max_iter, eps_sq, rel_prec, energy0, &iters));
  done(c, pf);
  return iters;
}
/* rat_monomial.c:232-250 on Qsw_pm_psi */
int tmlqcd_hip_cloverrat_acc(spinor *const pf, const double *mu, const double *rmu, const int np, const int max_iter, const double eps_sq,
                             const int rel_prec, double *energy1) {
  tmhip_ctx *c = ses.refresh_rat("tmlqcd_hip_cloverrat_acc");
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  int iters = -1;
  CK(tmhip_cloverrat_acc(c, f, mu, rmu, np, max_iter, eps_sq, rel_prec, energy1, &iters));
  return iters;
}

// ------------------------------------------------------------------ correction monomials (ratcor_monomial.c, ndratcor_monomial.c; rational.hip)
// heatbath: pf (pf2) are updated in place; acc only reads them.  All return the summed return values of the first solve of every Z.
static int ratcor_call(const char *who, bool heatbath, int op, spinor *const pf, const double *mu, const double *rmu, const double A, const int np,
                       const int max_iter, const double accprec, const int rel_prec, double *energy, int *napp) {
  tmhip_ctx *c = ses.refresh_rat(who);
  tmhip_field *f = in(c, pf, TMHIP_FIELD_EO);
  int iters = -1, n = 0;
  CK((heatbath ? tmhip_ratcor_heatbath : tmhip_ratcor_acc)(c, f, mu, rmu, A, np, max_iter, accprec, rel_prec, op, energy, &n, &iters));
  if (heatbath) done(c, pf);
  if (napp) *napp = n;
  return iters;
}
static int ndratcor_call(const char *who, bool heatbath, int op, spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A,
                         const int np, const int max_iter, const double accprec, const int rel_prec, double *energy, int *napp) {
  tmhip_ctx *c = ses.refresh_nd(who);
  tmhip_field *fu = in(c, pf, TMHIP_FIELD_EO), *fd = in(c, pf2, TMHIP_FIELD_EO);
  int iters = -1, n = 0;
  CK((heatbath ? tmhip_ndratcor_heatbath : tmhip_ndratcor_acc)(c, fu, fd, mu, rmu, A, np, max_iter, accprec, rel_prec, op, energy, &n, &iters));
  if (heatbath) { done(c, pf); done(c, pf2); }
  if (napp) *napp = n;
  return iters;
}
/* ratcor_monomial.c:85-110 */
int tmlqcd_hip_ratcor_heatbath(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                               const double accprec, const int rel_prec, double *energy0, int *napp) {
  return ratcor_call("tmlqcd_hip_ratcor_heatbath", true, TMHIP_OP_QTM_PM, pf, mu, rmu, A, np, max_iter, accprec, rel_prec, energy0, napp);
}
/* ratcor_monomial.c:151-168 */
int tmlqcd_hip_ratcor_acc(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter, const double accprec,
                          const int rel_prec, double *energy1, int *napp) {
  return ratcor_call("tmlqcd_hip_ratcor_acc", false, TMHIP_OP_QTM_PM, pf, mu, rmu, A, np, max_iter, accprec, rel_prec, energy1, napp);
}
/* type CLOVERRATCOR, after the caller's tmlqcd_hip_sw_term + tmlqcd_hip_sw_invert(EE, 0.) (:75-76,137-138) */
int tmlqcd_hip_cloverratcor_heatbath(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                                     const double accprec, const int rel_prec, double *energy0, int *napp) {
  return ratcor_call("tmlqcd_hip_cloverratcor_heatbath", true, TMHIP_OP_QSW_PM, pf, mu, rmu, A, np, max_iter, accprec, rel_prec, energy0, napp);
}
int tmlqcd_hip_cloverratcor_acc(spinor *const pf, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                                const double accprec, const int rel_prec, double *energy1, int *napp) {
  return ratcor_call("tmlqcd_hip_cloverratcor_acc", false, TMHIP_OP_QSW_PM, pf, mu, rmu, A, np, max_iter, accprec, rel_prec, energy1, napp);
}
/* ndratcor_monomial.c:88-123 */
int tmlqcd_hip_ndratcor_heatbath(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                 const int max_iter, const double accprec, const int rel_prec, double *energy0, int *napp) {
  return ndratcor_call("tmlqcd_hip_ndratcor_heatbath", true, TMHIP_ND_OP_QTM_PM, pf, pf2, mu, rmu, A, np, max_iter, accprec, rel_prec, energy0, napp);
}
/* ndratcor_monomial.c:166-187 */
int tmlqcd_hip_ndratcor_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np, const int max_iter,
                            const double accprec, const int rel_prec, double *energy1, int *napp) {
  return ndratcor_call("tmlqcd_hip_ndratcor_acc", false, TMHIP_ND_OP_QTM_PM, pf, pf2, mu, rmu, A, np, max_iter, accprec, rel_prec, energy1, napp);
}
/* type NDCLOVERRATCOR, after the caller's tmlqcd_hip_sw_term + sw_invert_nd(mubar^2 - epsbar^2) (:77-78,146-147) */
int tmlqcd_hip_ndcloverratcor_heatbath(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                       const int max_iter, const double accprec, const int rel_prec, double *energy0, int *napp) {
  return ndratcor_call("tmlqcd_hip_ndcloverratcor_heatbath", true, TMHIP_ND_OP_QSW_PM, pf, pf2, mu, rmu, A, np, max_iter, accprec, rel_prec, energy0, napp);
}
int tmlqcd_hip_ndcloverratcor_acc(spinor *const pf, spinor *const pf2, const double *mu, const double *rmu, const double A, const int np,
                                  const int max_iter, const double accprec, const int rel_prec, double *energy1, int *napp) {
  return ndratcor_call("tmlqcd_hip_ndcloverratcor_acc", false, TMHIP_ND_OP_QSW_PM, pf, pf2, mu, rmu, A, np, max_iter, accprec, rel_prec, energy1, napp);
}

// ------------------------------------------------------------------ molecular dynamics with the links in HBM
/* update_gauge(step, hf) (update_gauge.c:51-110): U <- restoresu3(exposu3(step P)) U for every link, on the device-resident
 * links; the stencil's gauge copy is re-sorted there too (update_backward_gauge.c:185-242), so an MD step moves no gauge
 * field over PCIe.  Coherent mode: hf->gaugefield receives the new links before the call returns and the reference's flags
 * are raised (update_gauge.c:104-106) -- the next stencil call refreshes the HOST's backward copy if the program has one, but
 * does not upload again.  Resident mode: g_gauge_field stays behind until tmlqcd_hip_sync_gauge_to_host.
 * The clover blocks become stale exactly as in the reference (the monomials call sw_term / sw_invert again). */
// Host links and device links have just been brought to the same state by a download.  update_gauge.c:104-106 raises the flags
// here and leaves the refresh of the host's backward copy to the next consumer; this library IS the next consumer of
// g_update_gauge_copy, and it must be able to tell its own raise from a later one by the host program (which means "my links
// changed: upload them").  So the host's backward copy is refreshed right away (update_backward_gauge clears the flag) and the
// flag stays down: whoever raises it afterwards forces an upload.  The host's fp32 copy is host business: its flag is raised.
static void links_in_step(su3 **gf, hamiltonian_field_t *hf) {
  if (update_backward_gauge) update_backward_gauge(gf);
  g_update_gauge_copy = 0;
  if (hf) hf->update_gauge_copy = 0;
  if (&g_update_gauge_copy_32) g_update_gauge_copy_32 = 1;
  ses.gauge_uploaded = true;
}
void tmlqcd_hip_update_gauge(const double step, hamiltonian_field_t *const hf) {
  tmhip_ctx *c = ses.refresh(true);                                 // first call of a trajectory: the host's links go up once
  if (!ses.momenta_resident) CK(tmhip_momenta_upload(c, &hf->momenta[0][0]));
  CK(tmhip_update_gauge(c, step));
  ses.clover_stale();
  if (!resident()) {
    CK(tmhip_gauge_download(c, &hf->gaugefield[0][0]));
    links_in_step(hf->gaugefield, hf);
  } else {
    ses.dev_links_newer = true;
  }
}
void tmlqcd_hip_sync_gauge_to_host(hamiltonian_field_t *const hf) {
  if (!ses.dev_links_newer) return;
  CK(tmhip_gauge_download(ctx(), &hf->gaugefield[0][0]));
  links_in_step(hf->gaugefield, hf);                              // host-side consumers find the backward copy current
  ses.dev_links_newer = false;
}
/* update_momenta.c:67-72 for a force that was accumulated on the device only (deriv_Sb / tmlqcd_hip_sw_all in resident mode,
 * not flushed): P -= step * derivative with both resident; the momenta then stay on the device until
 * tmlqcd_hip_sync_momenta_to_host.  Contributions other monomials left in hf->derivative are NOT included. */
void tmlqcd_hip_update_momenta(const double step, hamiltonian_field_t *const hf) {
  tmhip_ctx *c = ses.refresh(false);
  if (!ses.momenta_resident) { CK(tmhip_momenta_upload(c, &hf->momenta[0][0])); ses.momenta_resident = true; }
  CK(tmhip_update_momenta(c, step));
  ses.deriv_pending = false;                                        // consumed
}
void tmlqcd_hip_sync_momenta_to_host(hamiltonian_field_t *const hf) {
  if (!ses.momenta_resident) return;
  CK(tmhip_momenta_download(ctx(), &hf->momenta[0][0]));
  ses.momenta_resident = false;
}

// ------------------------------------------------------------------ the frame of a trajectory (update_tm.c around the integrator)
/* update_tm.c:109-121: gauge_tmp <- links, on the device */
void tmlqcd_hip_gauge_snapshot(hamiltonian_field_t *const hf) {
  (void)hf;
  CK(tmhip_gauge_snapshot(ses.refresh(true)));
}
/* moment_energy(hf->momenta) (moment_energy.c:46-89), MPI_Allreduce included */
double tmlqcd_hip_moment_energy(hamiltonian_field_t *const hf) {
  tmhip_ctx *c = ses.refresh(false);
  if (!ses.momenta_resident) CK(tmhip_momenta_upload(c, &hf->momenta[0][0]));
  CK(tmhip_set_option(c, "gauge_global_sums", 1));
  double e = 0.0;
  CK(tmhip_moment_energy(c, &e));
  return e;
}
/* update_tm.c:233-277: ret_gauge_diff */
double tmlqcd_hip_gauge_snapshot_diff(hamiltonian_field_t *const hf) {
  (void)hf;
  tmhip_ctx *c = ses.refresh(true);
  CK(tmhip_set_option(c, "gauge_global_sums", 1));
  double d = 0.0;
  CK(tmhip_gauge_snapshot_diff(c, &d));
  return d;
}
// update_tm.c:344-352 after the links changed on the device: the two sides are brought to the same state (coherent, lazy) or the device is
// marked ahead (resident); a flag the host raised in between belongs to links that no longer exist
static void links_after_acceptance(tmhip_ctx *c, hamiltonian_field_t *const hf) {
  ses.clover_stale();
  ses.momenta_resident = false;   // the trajectory is over: its momenta are not needed again (no download), the next one's are drawn on the host
  if (!resident()) {
    CK(tmhip_gauge_download(c, &hf->gaugefield[0][0]));
    links_in_step(hf->gaugefield, hf);
    ses.dev_links_newer = false;
  } else {
    g_update_gauge_copy = 0;
    hf->update_gauge_copy = 0;
    ses.gauge_uploaded = true;
    ses.dev_links_newer = true;
  }
}
/* update_tm.c:313-328 and :344-346 */
void tmlqcd_hip_accept_links(hamiltonian_field_t *const hf, const int reunitarize) {
  tmhip_ctx *c = ses.refresh(true);
  if (reunitarize) CK(tmhip_gauge_reunitarize(c));
  links_after_acceptance(c, hf);
}
/* update_tm.c:329-339 and :344-346 */
void tmlqcd_hip_reject_links(hamiltonian_field_t *const hf) {
  tmhip_ctx *c = ses.refresh(false);                                // (no upload: the snapshot replaces whatever the host's links are)
  CK(tmhip_gauge_restore(c));
  links_after_acceptance(c, hf);
}
void tmlqcd_hip_transfer_counts(unsigned long out[4]) {
  long long n[4] = {0, 0, 0, 0};
  if (ses.c) CK(tmhip_transfer_counts(ses.c, n));
  for (int k = 0; k < 4; k++) out[k] = (unsigned long)n[k];
}
/* monitor_forces.c:64-97 on the device's derivative accumulator */
void tmlqcd_hip_force_norms(hamiltonian_field_t *const hf, double *sum, double *max) {
  (void)hf;
  tmhip_ctx *c = ses.refresh(false);
  *sum = *max = 0.0;
  if (!ses.deriv_made) return;
  CK(tmhip_set_option(c, "gauge_global_sums", 1));
  CK(tmhip_derivative_norms(c, sum, max));
}

// ------------------------------------------------------------------ ILDG gauge configurations
/* io/gauge_read.c:26-27: the record read_gauge_field fills (defined by the object this library replaces) */
paramsGaugeInfo GaugeInfo = {0., 0, {0, 0}, NULL, NULL};

/* io/gauge_read.c:28-198 read_gauge_field(filename, gf): LIME records walked on the host, the binary record unpacked and
 * check-summed in HBM; gf (the host's g_gauge_field) is filled, GaugeInfo set, g_update_gauge_copy raised; returns 0 or -1 with the
 * reference's messages. */
int read_gauge_field(char *filename, su3 **const gf) {
  tmhip_ctx *c = ctx();      // (T-split ranks: every rank reads its part of the record, tmlqcd_hip_comm_init must have been called)
  ses.calls++;
  static tmhip_gauge_info info;
  const int prec = &gauge_precision_read_flag && gauge_precision_read_flag == 32 ? 32 : 64;
  const int checks = !(&g_disable_IO_checks && g_disable_IO_checks);
  GaugeInfo.gaugeRead = 0;
  const int rc = tmhip_read_gauge_field(c, filename, prec, checks, &gf[0][0], &info);
  if (rc == -1) return -1;
  if (rc != 0) die("tmhip_read_gauge_field");
  GaugeInfo.gaugeRead = info.gauge_read;
  GaugeInfo.checksum.suma = info.suma; GaugeInfo.checksum.sumb = info.sumb;
  if (info.xlf_info[0]) { free(GaugeInfo.xlfInfo); GaugeInfo.xlfInfo = strdup(info.xlf_info); }
  if (info.ildg_data_lfn[0]) { free(GaugeInfo.ildg_data_lfn); GaugeInfo.ildg_data_lfn = strdup(info.ildg_data_lfn); }
  g_update_gauge_copy = 1;                                          /* gauge_read.c:190 */
  ses.clover_stale();
  // (the flag stays raised exactly as the reference leaves it: the host program still has its xchange_gauge to do, and the next
  // operator call uploads g_gauge_field once more -- 11 ms per configuration read at 32^4 -- rather than guess that nothing changed)
  if (gf == g_gauge_field && info.gauge_read) ses.dev_links_newer = false;
  return 0;
}

/* io/gauge_write.c:22-59 write_gauge_field(filename, prec, xlfInfo): the records of the reference in its order; the binary record and
 * its checksum come from the links in HBM (uploaded from g_gauge_field first unless the device copy is the current one) */
int write_gauge_field(char *filename, const int prec, paramsXlfInfo const *xlfInfo) {
  if (g_nproc_t > 1) die("write_gauge_field: single-rank writer (T-split ranks: tmhip_gauge_pack_ildg for their part of the record)");
  tmhip_ctx *c = ctx();
  ses.calls++;
  if (!ses.dev_links_newer) { CK(tmhip_set_gauge(c, &g_gauge_field[0][0])); ses.gauge_uploaded = true; ses.clover_stale(); }
  char msg[1024];
  msg[0] = 0;
  if (xlfInfo) {                                                    /* io/utils_write_xlf.c:35-55: plain text, what write_gauge_field (io/gauge_write.c:35) writes */
    if (xlfInfo->kappa != 0.0)
      snprintf(msg, sizeof(msg), "plaquette = %14.12f\n trajectory nr = %d\n beta = %.12f, kappa = %.12f, mu = %.12f, c2_rec = %f\n time = %ld\n"
               " hmcversion = %s\n mubar = %.12f\n epsilonbar = %.12f\n date = %s",
               xlfInfo->plaq, xlfInfo->counter, xlfInfo->beta, xlfInfo->kappa, xlfInfo->mu, xlfInfo->c2_rec, xlfInfo->time, xlfInfo->package_version,
               xlfInfo->mubar, xlfInfo->epsilonbar, xlfInfo->date);
    else
      snprintf(msg, sizeof(msg), "plaquette = %e\n trajectory nr = %d\n beta = %.12f\n kappa = %.12f\n 2*kappa*mu = %.12f\n c2_rec = %f\n date = %s",
               xlfInfo->plaq, xlfInfo->counter, xlfInfo->beta, xlfInfo->kappa, xlfInfo->mu, xlfInfo->c2_rec, xlfInfo->date);
  }
  unsigned cs[2];
  return tmhip_write_gauge_field(c, filename, prec, msg[0] ? msg : nullptr, cs) ? -1 : 0;
}

// ------------------------------------------------------------------ propagators and sources
/* The e/o pair (s, r) or -- r == NULL -- the lexicographic field s as the two one-parity device fields the core calls take */
static void spinor_pair(tmhip_ctx *c, spinor *s, spinor *r, bool reading, tmhip_field **fe, tmhip_field **fo) {
  if (r) {
    *fe = reading ? in(c, s, TMHIP_FIELD_EO) : out(c, s, TMHIP_FIELD_EO);
    *fo = reading ? in(c, r, TMHIP_FIELD_EO) : out(c, r, TMHIP_FIELD_EO);
  } else {
    tmhip_field *f = reading ? in(c, s, TMHIP_FIELD_FULL) : out(c, s, TMHIP_FIELD_FULL);
    *fe = tmhip_field_even(f); *fo = tmhip_field_odd(f);
  }
}

/* io/spinor_read.c:27-150 read_spinor(s, r, filename, position): the LIME records are walked on the host, the record goes through
 * page-locked memory to the device and is unpacked and check-summed there; (s, r) follow the residency mode like any other output.
 * r == NULL: s is a lexicographic field of VOLUME sites (read_binary_spinor_data_l).  Return values, messages and prints are the
 * reference's; a file that is refused leaves s and r as they were. */
int read_spinor(spinor *const s, spinor *const r, char *filename, const int position) {
  if (g_nproc_t > 1) die("read_spinor: single-rank reader (T-split ranks: tmhip_spinor_unpack for their part of the record)");
  tmhip_ctx *c = ctx();
  ses.calls++;
  tmhip_field *fe, *fo;
  spinor_pair(c, s, r, false, &fe, &fo);
  tmhip_spinor_info info;
  const int checks = !(&g_disable_src_IO_checks && g_disable_src_IO_checks == 1);
  const bool talk = (&g_cart_id ? g_cart_id : 0) == 0 && (&g_debug_level ? g_debug_level : 1) >= 0;
  const int rc = tmhip_read_spinor(c, fe, fo, filename, position, checks, &info);
  if (rc > 0) die("tmhip_read_spinor");
  if (talk && info.prec) printf("# %s precision read (%d bits).\n", info.prec == 64 ? "Double" : "Single", info.prec);   /* spinor_read.c:97-99: before the data */
  if (rc < 0) return rc;
  done(c, s);
  if (r) done(c, r);
  if (talk) {
    if (checks) {
      printf("# Scidac checksums for DiracFermion field %s position %d:\n", filename, info.position);
      printf("#   Calculated            : A = %#010x B = %#010x.\n", info.suma, info.sumb);
      printf("#   Read from LIME headers: A = %#010x B = %#010x.\n", info.suma_stored, info.sumb_stored);
    }
  }
  return 0;
}

/* What write_spinor (io/spinor_write.c:23-47) puts on a writer, on a file name: the reference's function takes a c-lime WRITER and
 * cannot be replaced under its own name.  A host array whose device mirror is current is packed where it lies; any other is
 * uploaded first.  r == NULL: s[i] are lexicographic fields.  Returns 0, or -1 after a message. */
int tmlqcd_hip_write_spinor(char *filename, const int append, spinor **const s, spinor **const r, const int flavours, const int prec) {
  if (g_nproc_t > 1) die("tmlqcd_hip_write_spinor: single-rank writer (T-split ranks: tmhip_spinor_pack for their part of the record)");
  if (flavours < 1 || flavours > 8) die("tmlqcd_hip_write_spinor: 1 to 8 flavours");
  tmhip_ctx *c = ctx();
  ses.calls++;
  tmhip_field *fe[8], *fo[8];
  for (int i = 0; i < flavours; i++) spinor_pair(c, s[i], r ? r[i] : nullptr, true, &fe[i], &fo[i]);
  return tmhip_write_spinor(c, filename, append, fe, fo, flavours, prec, nullptr) ? -1 : 0;
}
int tmlqcd_hip_write_lime_message(char *filename, const int append, const char *type, const char *text, const int mb, const int me) {
  return tmhip_write_lime_message(filename, append, type, text, mb, me) ? -1 : 0;
}

/* start.c:707-741 and start.c:743-830 on the device mirrors of P and Q (start.o keeps the random number generator and stays on the
 * link line, so these carry names of their own) */
void tmlqcd_hip_source_spinor_field_point_from_file(spinor *const P, spinor *const Q, int is, int ic, int source_indx) {
  tmhip_ctx *c = ctx();
  ses.calls++;
  const long long Vg = (long long)VOLUME * (g_nproc_t < 1 ? 1 : g_nproc_t);
  if (source_indx < 0 || source_indx >= Vg) {     /* start.c:755-759 */
    printf("Error in the input parameter file, SourceLocation must be in [0,VOLUME-1]! Exiting...!\n");
    exit(1);
  }
  tmhip_field *fp = out(c, P, TMHIP_FIELD_EO), *fq = out(c, Q, TMHIP_FIELD_EO);
  CK(tmhip_source_point(c, fp, fq, is, ic, source_indx));
  done(c, P); done(c, Q);
}
void tmlqcd_hip_source_spinor_field(spinor *const P, spinor *const Q, int is, int ic) {
  tmlqcd_hip_source_spinor_field_point_from_file(P, Q, is, ic, 0);
}

// ------------------------------------------------------------------ benchmark helper
/* benchmark.c:291-300 with the three fields resident in HBM */
double tmlqcd_hip_benchmark_loop(spinor *f0, spinor *f1, spinor *f2, int iters) {
  tmhip_ctx *c = ses.refresh(true);
  bench_begin();
  tmhip_field *d0 = in(c, f0, TMHIP_FIELD_EO), *d1 = out(c, f1, TMHIP_FIELD_EO), *d2 = out(c, f2, TMHIP_FIELD_EO);
  double ms = 0;
  CK(tmhip_bench_hopping(c, d0, d1, d2, iters, &ms));
  bench_finish(c, f1, f2);
  return ms * 1e-3;
}

}  // extern "C"

// ------------------------------------------------------------------ the generic host loops of cg_her and cg_mms_tm
namespace {

// generic path of cg_her: reference algorithm verbatim on host-visible fields
int cg_her_generic(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N, matrix_mult f) {
  CoherentScope coherent;
  const size_t Vf = (size_t)(N == VOLUME ? VOLUMEPLUSRAND : VOLUMEPLUSRAND / 2);
  spinor *blk = (spinor *)calloc(3 * Vf + 1, sizeof(spinor));   /* solver_field.c:31-71 */
  if (!blk) die("cg_her: out of memory");
  spinor *sf[3] = {blk, blk + Vf, blk + 2 * Vf}, *stmp;
  double normsq, pro, err, alpha_cg, beta_cg, squarenorm;
  int iteration;
  squarenorm = square_norm(Q, N, 1);
  f(sf[0], P);
  diff(sf[1], Q, sf[0], N);
  assign(sf[2], sf[1], N);
  normsq = square_norm(sf[1], N, 1);
  for (iteration = 1; iteration <= max_iter; iteration++) {
    f(sf[0], sf[2]);
    pro = scalar_prod_r(sf[2], sf[0], N, 1);
    alpha_cg = normsq / pro;
    assign_add_mul_r(P, sf[2], alpha_cg, N);
    err = assign_mul_add_r_and_square(sf[0], -alpha_cg, sf[1], N, 1);
    if (((err <= eps_sq) && (rel_prec == 0)) || ((err <= eps_sq * squarenorm) && (rel_prec == 1))) break;
    beta_cg = err / normsq;
    assign_mul_add_r(sf[2], beta_cg, sf[0], N);
    stmp = sf[0]; sf[0] = sf[1]; sf[1] = stmp;
    normsq = err;
  }
  for (int i = 0; i < 3; i++) tmlqcd_hip_forget(blk + i * Vf);  // addresses are about to be recycled
  free(blk);
  if (iteration > max_iter) return -1;
  return iteration;
}

// generic path of bicgstab_complex: the reference's statements on host-visible fields
int bicgstab_complex_generic(spinor *const P, spinor *const Q, const int max_iter, double eps_sq, const int rel_prec, const int N, matrix_mult f) {
  CoherentScope coherent;
  const size_t Vf = (size_t)(N == VOLUME ? VOLUMEPLUSRAND : VOLUMEPLUSRAND / 2);
  spinor *blk = (spinor *)calloc(6 * Vf + 1, sizeof(spinor));   /* solver_field.c:31-71 */
  if (!blk) die("bicgstab_complex: out of memory");
  spinor *hatr = blk, *r = blk + Vf, *v = blk + 2 * Vf, *p = blk + 3 * Vf, *s = blk + 4 * Vf, *t = blk + 5 * Vf;
  int ret = -1;
  f(r, P);
  diff(p, Q, r, N);
  assign(r, p, N);
  assign(hatr, p, N);
  _Complex double rho0 = scalar_prod(hatr, r, N, 1);
  const double squarenorm = square_norm(Q, N, 1);
  for (int i = 0; i < max_iter; i++) {
    const double err = square_norm(r, N, 1);
    if ((((err <= eps_sq) && (rel_prec == 0)) || ((err <= eps_sq * squarenorm) && (rel_prec == 1))) && i > 0) { ret = i; break; }
    f(v, p);
    const _Complex double alpha = rho0 / scalar_prod(hatr, v, N, 1);
    assign(s, r, N);
    assign_diff_mul(s, v, alpha, N);
    f(t, s);
    _Complex double omega = scalar_prod(t, s, N, 1);
    omega /= square_norm(t, N, 1);
    assign_add_mul_add_mul(P, p, s, alpha, omega, N);
    assign(r, s, N);
    assign_diff_mul(r, t, omega, N);
    const _Complex double rho1 = scalar_prod(hatr, r, N, 1);
    if (fabs(__real__ rho1) < 1.e-25 && fabs(__imag__ rho1) < 1.e-25) break;
    const _Complex double beta = (alpha * rho1) / (omega * rho0);
    assign_mul_bra_add_mul_ket_add(p, v, r, -omega, beta, N);
    rho0 = rho1;
  }
  for (int i = 0; i < 6; i++) tmlqcd_hip_forget(blk + i * Vf);  // addresses are about to be recycled
  free(blk);
  return ret;
}

// chrono_guess with an operator the library does not know: f runs on host arrays, so everything around it runs in coherent mode, one
// drop-in linalg call at a time (the residency rules of cg_her_generic).  The steps are those of tmhip_chrono_guess and the small
// system is solved by the same function (tmhip_csg_solve).
int chrono_guess_generic(spinor *const trial, spinor *const phi, spinor **const v, const int *index_array, const int n, const int V, matrix_mult f) {
  CoherentScope coherent;
  spinor *newest = v[index_array[n - 1]];
  for (int i = n - 2; i >= 0; i--) assign_diff_mul(v[index_array[i]], newest, scalar_prod(newest, v[index_array[i]], V, 1), V);
  double G[2 * 20 * 20], b[2 * 20];
  for (int j = 0; j < n; j++) {
    f(trial, v[index_array[j]]);
    for (int i = 0; i <= j; i++) {
      const _Complex double s = scalar_prod(v[index_array[i]], trial, V, 1);
      G[2 * (i * n + j)] = __real__ s; G[2 * (i * n + j) + 1] = __imag__ s;
      G[2 * (j * n + i)] = __real__ s; G[2 * (j * n + i) + 1] = i == j ? __imag__ s : -__imag__ s;
    }
    const _Complex double s = scalar_prod(v[index_array[j]], phi, V, 1);
    b[2 * j] = __real__ s; b[2 * j + 1] = __imag__ s;
  }
  CK(tmhip_csg_solve(n, G, b));
  _Complex double y;
  __real__ y = b[2 * (n - 1)]; __imag__ y = b[2 * (n - 1) + 1];
  mul(trial, y, newest, V);
  for (int i = n - 2; i >= 0; i--) {
    __real__ y = b[2 * i]; __imag__ y = b[2 * i + 1];
    assign_add_mul(trial, v[index_array[i]], y, V);
  }
  return 0;
}

// generic path of cg_mms_tm: the reference loop verbatim on host-visible fields (assign_mul_add_mul_r inlined: the host program need not have it)
int cg_mms_tm_generic(spinor **const P, spinor *const Q, tmlqcd_solver_params *sp, double *cgmms_reached_prec) {
  const int N = sp->sdim, n = sp->no_shifts, max_iter = sp->max_iter, rel_prec = sp->rel_prec;
  const double eps_sq = sp->squared_solver_prec;
  CoherentScope coherent;
  const size_t Vf = (size_t)(N == VOLUME ? VOLUMEPLUSRAND : VOLUMEPLUSRAND / 2);
  const int ns = n > 1 ? n : 1;
  spinor *blk = (spinor *)calloc((3 + (size_t)(ns - 1)) * Vf + 1, sizeof(spinor));   /* solver_field.c:31-71, init_mms_tm :207-228 */
  double *co = (double *)calloc(5 * (size_t)ns, sizeof(double));
  if (!blk || !co) die("cg_mms_tm: out of memory");
  spinor *sf[3] = {blk, blk + Vf, blk + 2 * Vf};
  spinor **ps = (spinor **)calloc(ns, sizeof(spinor *));
  if (!ps) die("cg_mms_tm: out of memory");
  for (int s = 1; s < ns; s++) ps[s] = blk + (2 + s) * Vf;
  double *sigma = co, *zitam1 = co + ns, *zita = co + 2 * ns, *alphas = co + 3 * ns, *betas = co + 4 * ns;
  int no_shifts = n, iteration;
  double normsq, pro, err = 0.0, squarenorm, gamma, alpham1;
  for (int i = 0; i < N; i++) P[0][i] = spinor{};
  alphas[0] = 1.0; betas[0] = 0.0;
  sigma[0] = sp->shifts[0] * sp->shifts[0];
  for (int im = 1; im < no_shifts; im++) {
    sigma[im] = sp->shifts[im] * sp->shifts[im] - sigma[0];
    for (int i = 0; i < N; i++) P[im][i] = spinor{};
    assign(ps[im], Q, N);
    zitam1[im] = zita[im] = alphas[im] = 1.0; betas[im] = 0.0;
  }
  squarenorm = square_norm(Q, N, 1);
  assign(sf[0], Q, N);
  assign(sf[1], Q, N);
  normsq = squarenorm;
  for (iteration = 0; iteration < max_iter; iteration++) {
    sp->M_psi(sf[2], sf[1]);
    assign_add_mul_r(sf[2], sf[1], sigma[0], N);
    pro = scalar_prod_r(sf[1], sf[2], N, 1);
    alpham1 = alphas[0];
    alphas[0] = normsq / pro;
    for (int im = 1; im < no_shifts; im++) {
      gamma = zita[im] * alpham1 / (alphas[0] * betas[0] * (1. - zita[im] / zitam1[im]) + alpham1 * (1. + sigma[im] * alphas[0]));
      zitam1[im] = zita[im];
      zita[im] = gamma;
      alphas[im] = alphas[0] * zita[im] / zitam1[im];
      assign_add_mul_r(P[im], ps[im], alphas[im], N);
      if (iteration > 0 && (iteration % 20 == 0) && (im == no_shifts - 1)) {
        const double sn = square_norm(ps[im], N, 1);
        if (alphas[no_shifts - 1] * alphas[no_shifts - 1] * sn <= eps_sq) no_shifts--;
      }
    }
    assign_add_mul_r(P[0], sf[1], alphas[0], N);
    assign_add_mul_r(sf[0], sf[2], -alphas[0], N);
    err = square_norm(sf[0], N, 1);
    if (((err <= eps_sq) && (rel_prec == 0)) || ((err <= eps_sq * squarenorm) && (rel_prec > 0)) || (iteration == max_iter - 1)) {
      *cgmms_reached_prec = err;
      break;
    }
    betas[0] = err / normsq;
    assign_mul_add_r(sf[1], betas[0], sf[0], N);
    normsq = err;
    for (int im = 1; im < no_shifts; im++) {
      betas[im] = betas[0] * zita[im] * alphas[im] / (zitam1[im] * alphas[0]);
      const double c1 = betas[im], c2 = zita[im];   /* assign_mul_add_mul_r(ps, sf0, c1, c2, N) */
      double *r = (double *)ps[im];
      const double *s = (const double *)sf[0];
      for (size_t k = 0; k < (size_t)N * 24; k++) r[k] = c1 * r[k] + c2 * s[k];
    }
  }
  for (int i = 0; i < 3 + ns - 1; i++) tmlqcd_hip_forget(blk + (size_t)i * Vf);   // addresses are about to be recycled
  free(blk); free(co); free(ps);
  return iteration == max_iter - 1 ? -1 : iteration + 1;
}

}  // namespace
