// What the translation units of libtmlqcd_dropin.so share: the forwarding of the reference-named symbols (dropin.cpp) sees the
// mirror registry and the lazy-coherence machinery (residency.cpp) through this header only.  Nothing declared here becomes a dynamic
// symbol: the library is loaded RTLD_GLOBAL next to host programs that have an `in`, `out`, `done`, `ctx` or `die` of their own.
#ifndef TMLQCD_DROPIN_INTERNAL_H
#define TMLQCD_DROPIN_INTERNAL_H
#include "../../include/tmlqcd_dropin.h"
#include "../../include/tmlqcd_hip.h"
#include "op_table.h"

#include <cstddef>

extern "C" {
extern int VOLUME;   /* global.h:82-84, owned by the host program */
}

#pragma GCC visibility push(hidden)

// Third mirror shape next to the two field kinds of the core library: the first `n` spinors of a host array taken as a plain
// sequence (the reference's linalg and site-diagonal routines loop over ANY 0 <= N; tests/test_linalg_spinor.c uses N = 2 and
// 1000, block solvers use block volumes).  Stored in a FULL-sized device field without the lexicographic <-> e/o permutation:
// sites [0, VOLUME/2) in its first half, [VOLUME/2, n) in its second.
#define KIND_LIN 2

[[noreturn]] void die(const char *what);
#define CK(call) do { if ((call) != 0) die(#call); } while (0)

// The element-wise routines work part by part: one part for a one-parity field or a short prefix, two for a FULL field (its two
// halves) or a prefix longer than VOLUME/2.
struct Parts { int n; int cnt[2]; };
inline Parts parts_of(int kind, int N) {
  const int Vh = VOLUME / 2;
  if (kind == TMHIP_FIELD_EO) return {1, {Vh, 0}};
  if (kind == TMHIP_FIELD_FULL) return {2, {Vh, Vh}};
  if (N <= Vh) return {1, {N, 0}};
  return {2, {Vh, N - Vh}};
}

// ---- dropin.cpp: the session's context
tmhip_ctx *ctx();        // made on first use from the host program's globals
tmhip_ctx *live_ctx();   // the same, or null before the first call and after tmlqcd_hip_finalize (all the fault handler may ask)

// ---- residency.cpp: host array -> device mirror
tmhip_field *in(tmhip_ctx *c, const void *host, int kind, int n = 0);    // operand read by the device: uploaded unless its mirror is current
tmhip_field *out(tmhip_ctx *c, const void *host, int kind, int n = 0);   // operand only written by the device
void done(tmhip_ctx *c, const void *host);                               // the device wrote it: download / close / keep, by the mode
int residency_mode();
inline bool resident() { return residency_mode() == TMLQCD_HIP_RESIDENT; }
void residency_from_env();                  // TMLQCD_HIP_RESIDENCY, read once when the context is made
void release_all_mirrors(tmhip_ctx *c);     // tmlqcd_hip_finalize: host copies current, then every mirror, pinned buffer and the watch table gone
// The generic host loops of cg_her / cg_mms_tm run in coherent mode.  Leaving restores the mode by plain assignment, NOT through
// tmlqcd_hip_set_residency: the setter would release and invalidate mirrors that are to be left alone.
struct CoherentScope {
  CoherentScope();
  ~CoherentScope();
  CoherentScope(const CoherentScope &) = delete;
 private:
  int saved;
};
// tmlqcd_hip_benchmark_loop: bench_begin() takes the registry's lock and forces the mode to resident; bench_finish() marks f1 and f2
// device-only, restores the mode, downloads, unwatches or closes the two as that mode asks, and gives the lock back.
void bench_begin();
void bench_finish(tmhip_ctx *c, spinor *f1, spinor *f2);

#pragma GCC visibility pop
#endif
