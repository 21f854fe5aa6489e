// libtmlqcd_dropin.so, residency half -- everything that knows what a mirror is: the registry host-pointer -> device mirror, the three
// residency modes, and the lazy-coherence machinery (SIGSEGV handler, page protection, page moves).  Opt-in and frozen: the forwarding
// of the reference-named symbols (dropin.cpp) reaches it through dropin_internal.h only, and no such symbol is defined here.
#include "dropin_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <unordered_map>
#include <vector>

#include <atomic>
#include <cerrno>
#include <dlfcn.h>
#include <fcntl.h>
#include <pthread.h>
#include <signal.h>
#include <stdint.h>
#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>

[[noreturn]] void die(const char *what) {
  fprintf(stderr, "[tmlqcd_dropin] fatal: %s\n", what);
  exit(1);  // the reference's error convention (fatal_error.c)
}

namespace {

struct Mirror {
  tmhip_field *f = nullptr;
  int kind = TMHIP_FIELD_EO;
  int n = 0;                // KIND_LIN: number of sites mirrored
  bool dev_valid = false;   // device copy holds the current data
  bool host_valid = true;   // host copy holds the current data
  unsigned long long last_use = 0;
  // lazy mode (TMLQCD_HIP_LAZY): the host array's pages are protected so that the host's own loads and stores say when a copy is needed
  size_t bytes = 0;         // extent of the host array this mirror stands for
  int prot = 0;             // P_RW: untouched; P_RO: both copies current, a host store must be noticed; P_NONE: the host copy is stale
  std::vector<unsigned char> page_ok;   // P_NONE: pages of the span already brought up to date one by one.  Sized ONCE, when the mirror is made
                                        // (lazy mode): the SIGSEGV handler and everything it calls only ever overwrite it
  int faults = 0;           // page-wise read synchronisations since the device last wrote the field
  bool nowatch = false;     // lazy mode: this array cannot be watched (malloc heap / arena, shared or file-backed mapping) -- never protected, copied per call like the coherent mode
  bool classified = false;  // lazy mode: nowatch / unsafe were decided
  bool unsafe = false;      // test hook TMLQCD_HIP_LAZY_FORCE_WATCH: watched although unwatchable -- a fault on it ends the program with a message (never a hang)
};
enum { P_RW = 0, P_RO = 1, P_NONE = 2 };
unsigned long long g_tick = 0;
size_t g_mirror_cap = 64;   // TMLQCD_HIP_MAX_MIRRORS: host programs that allocate work fields per solve (solver_field.c) would otherwise
                            // grow the registry without bound; mirrors whose host copy is current can be dropped at any time

int g_mode = TMLQCD_HIP_COHERENT;
std::unordered_map<const void *, Mirror> g_reg;
// What the SIGSEGV handler of the lazy mode walks instead of the map: a fixed array of (host array, its mirror) kept in step with g_reg
// under the lock (mirrors live in map nodes: their addresses are stable).  Reading it allocates nothing and follows no bucket chain.
struct Watch { const void *host; Mirror *m; };
constexpr int WATCH_CAP = 4096;
Watch g_watch[WATCH_CAP];
int g_nwatch = 0;

// ONE lock for the registry: taken around every change of g_reg or of a mirror's state by the entry points and for the whole body of
// the SIGSEGV handler of the lazy mode, which walks the map -- a host thread faulting on a stale field while the master thread is
// inside a drop-in call must never see a rehash in progress.  Recursive per thread (mirror() -> evict; a fault of the thread that
// holds it, e.g. in the memcpy of an upload, is served in place: no structural change is in progress then).  A spin lock: pthread
// mutexes are not async-signal-safe.  The owner's thread id IS the lock word (0: free): "do I hold it already" is then one atomic
// load that only the asking thread itself can have made true -- an owner id kept next to a separate flag can be read stale by a
// thread that held the lock before, which then walks in beside the new owner.
std::atomic<uintptr_t> g_reg_owner(0);
int g_reg_depth = 0;                              // touched by the owner only
inline void reg_lock() {
  const uintptr_t me = (uintptr_t)pthread_self();
  if (g_reg_owner.load(std::memory_order_relaxed) == me) { g_reg_depth++; return; }
  uintptr_t expected = 0;
  while (!g_reg_owner.compare_exchange_weak(expected, me, std::memory_order_acquire)) { expected = 0; __builtin_ia32_pause(); }
  g_reg_depth = 1;
}
inline void reg_unlock() {
  if (--g_reg_depth == 0) g_reg_owner.store(0, std::memory_order_release);
}
struct RegLock {
  RegLock() { reg_lock(); }
  ~RegLock() { reg_unlock(); }
};

int nsites(int kind) { return kind == TMHIP_FIELD_FULL ? VOLUME : VOLUME / 2; }

// ------------------------------------------------------------------ lazy coherence (TMLQCD_HIP_LAZY)
// An UNMODIFIED host program keeps its fields in HBM: after a device operation wrote a field, the pages of the host array are made
// inaccessible; the host's first load from one of them faults, the handler brings that page up to date from the device mirror (a few
// microseconds: 21 spinors) and lets the load go on -- or the whole field once the host keeps reading (more than LAZY_PAGE_FAULTS pages)
// or stores to it.  After an upload the pages are read-only, so a host store invalidates the mirror.  benchmark.c's loop (it reads one
// number of the output per iteration, :291-300) then runs at the resident rate with no source change.  Limits, hence opt-in: the
// kernel does not raise SIGSEGV for its own accesses -- a field handed to write(2) / MPI while its host copy is stale fails with
// EFAULT instead of being synchronised (tmlqcd_hip_sync_to_host first); pages shared with neighbouring data are handled, at the price
// of a synchronisation when that data is touched.
#define LAZY_PAGE_FAULTS 8
uintptr_t g_page = 4096;
struct sigaction g_old_segv;
bool g_handler_installed = false;
std::atomic<uintptr_t> g_handler_thread(0);       // the thread the SIGSEGV handler is running on (0: none) -- one word, see RegLock
inline bool in_handler_here() { return g_handler_thread.load(std::memory_order_relaxed) == (uintptr_t)pthread_self(); }
unsigned long g_lazy_stats[4] = {0, 0, 0, 0};   // faults served, pages fetched one by one, whole-field fetches, stores noticed (tmlqcd_hip_lazy_stats)

inline uintptr_t span_lo(const void *h) { return (uintptr_t)h & ~(g_page - 1); }
inline uintptr_t span_hi(const void *h, size_t bytes) { return ((uintptr_t)h + bytes + g_page - 1) & ~(g_page - 1); }
inline int prot_flags(int p) { return p == P_RW ? (PROT_READ | PROT_WRITE) : (p == P_RO ? PROT_READ : PROT_NONE); }
// what mirror m asks for page `page` of its span
inline int page_want(const void *host, const Mirror &m, uintptr_t page) {
  if (m.prot != P_NONE) return m.prot;
  const size_t idx = (page - span_lo(host)) / g_page;
  return idx < m.page_ok.size() && m.page_ok[idx] ? P_RO : P_NONE;
}
// the strictest protection any mirror asks for this page (pages at the edge of a field are shared with its neighbours)
int page_need(uintptr_t page, const std::unordered_map<const void *, Mirror> & /* the watch table mirrors it */) {
  int need = P_RW;
  for (int k = 0; k < g_nwatch; k++) {
    const Mirror &m = *g_watch[k].m;
    const void *host = g_watch[k].host;
    if (m.prot == P_RW || !m.bytes) continue;
    if (page < span_lo(host) || page >= span_hi(host, m.bytes)) continue;
    const int w = page_want(host, m, page);
    if (w > need) need = w;
  }
  return need;
}
// g_reg changed (insert / erase): bring the handler's table in step.  Entry-point context, under the lock.
void rebuild_watch() {
  g_nwatch = 0;
  for (auto &kv : g_reg) {
    if (g_nwatch == WATCH_CAP) { fprintf(stderr, "[tmlqcd_dropin] fatal: more than %d mirrored host arrays\n", WATCH_CAP); exit(1); }
    g_watch[g_nwatch++] = Watch{kv.first, &kv.second};
  }
}
// (re)apply the protection of one mirror's span; interior pages belong to it alone, the two edge pages are negotiated
void apply_prot(const void *host, Mirror &m, const std::unordered_map<const void *, Mirror> &reg) {
  if (!m.bytes) return;
  const uintptr_t lo = span_lo(host), hi = span_hi(host, m.bytes);
  for (uintptr_t pg = lo; pg < hi; pg += g_page) {
    const bool edge = pg < (uintptr_t)host || pg + g_page > (uintptr_t)host + m.bytes;
    if (edge) { mprotect((void *)pg, g_page, prot_flags(page_need(pg, reg))); continue; }
    // run of interior pages with the same wish
    const int w = page_want(host, m, pg);
    uintptr_t end = pg + g_page;
    while (end < hi && end + g_page <= (uintptr_t)host + m.bytes && page_want(host, m, end) == w) end += g_page;
    mprotect((void *)pg, end - pg, prot_flags(w));
    pg = end - g_page;
  }
}
void set_prot(const void *host, Mirror &m, int prot, const std::unordered_map<const void *, Mirror> &reg) {
  if (m.prot == prot && prot != P_NONE) return;
  if (m.prot == P_NONE && prot == P_NONE) {
    // the device wrote the field again while the host copy was already closed: only the pages the host had fetched in between
    // need closing (none at all in a loop of device calls -- an mprotect over the whole 100 MB span costs milliseconds)
    if (m.faults == 0) return;
    const uintptr_t lo = span_lo(host);
    for (size_t i = 0; i < m.page_ok.size(); i++)
      if (m.page_ok[i]) { m.page_ok[i] = 0; mprotect((void *)(lo + i * g_page), g_page, prot_flags(page_need(lo + i * g_page, reg))); }
    m.faults = 0;
    return;
  }
  m.prot = prot;
  const size_t npages = (span_hi(host, m.bytes) - span_lo(host)) / g_page;
  if (prot == P_NONE && m.page_ok.size() != npages) m.page_ok.assign(npages, 0);   // (entry points only: the handler never closes a span)
  else std::fill(m.page_ok.begin(), m.page_ok.end(), 0);
  if (prot == P_NONE) m.faults = 0;
  apply_prot(host, m, reg);
}

// Lazy mode never lets the runtime touch the program's own pages: a copy from / to pageable memory registers those pages with the
// driver, and every later mprotect on them goes through its MMU notifier (measured: 28 ms per call instead of microseconds).  Data
// moves through a page-locked bounce buffer instead; uploads and whole-field downloads are the rare events in this mode.
// Two of them: the entry points' and the fault handler's.  An upload copies host -> bounce with memcpy, and that copy can itself
// fault (an edge page shared with a neighbouring field whose host copy is stale, a stale mirror overlapping the span); the handler's
// whole-field download of that neighbour must not land in -- or re-allocate -- the buffer the interrupted copy is filling.
void *g_bounce[2] = {nullptr, nullptr};
size_t g_bounce_bytes[2] = {0, 0};
void *g_page_tmp = nullptr;     // page-locked: the handler's page-wise fetches (64 spinors)
[[noreturn]] void handler_die(const char *msg) {   // async-signal-safe exit with a message
  (void)!write(2, msg, strlen(msg));
  _exit(1);
}
void *bounce(size_t bytes) {
  const int k = in_handler_here() ? 1 : 0;
  if (k == 1 && g_bounce_bytes[1] < bytes) handler_die("[tmlqcd_dropin] fatal: lazy mode: the fault handler's staging buffer is smaller than the field it has to fetch\n");
  if (g_bounce_bytes[k] < bytes) {
    if (g_bounce[k]) tmhip_pinned_free(g_bounce[k]);
    g_bounce[k] = nullptr; g_bounce_bytes[k] = 0;
    CK(tmhip_pinned_alloc(bytes, &g_bounce[k]));
    g_bounce_bytes[k] = bytes;
  }
  return g_bounce[k];
}

// Called by mirror() in lazy mode (entry-point context): whatever the fault handler will need for an array of this size exists before
// the array is ever watched -- its page-locked staging buffer, the page buffer.  The handler allocates nothing.
void prepare_handler_buffers(size_t bytes) {
  if (g_bounce_bytes[1] < bytes) {
    if (g_bounce[1]) tmhip_pinned_free(g_bounce[1]);
    g_bounce[1] = nullptr; g_bounce_bytes[1] = 0;
    CK(tmhip_pinned_alloc(bytes, &g_bounce[1]));
    g_bounce_bytes[1] = bytes;
  }
  if (!g_page_tmp) CK(tmhip_pinned_alloc(64 * sizeof(spinor), &g_page_tmp));
}

// host <-> device for a mirror of any shape (KIND_LIN: the two halves are plain prefixes, no site permutation)
void upload(tmhip_ctx *c, const void *host_user, Mirror &m) {
  const void *host = host_user;
  if (g_mode == TMLQCD_HIP_LAZY) { void *b = bounce(m.bytes); memcpy(b, host_user, m.bytes); host = b; }
  if (m.kind != KIND_LIN) { CK(tmhip_field_upload(c, m.f, host, nsites(m.kind))); return; }
  const Parts pt = parts_of(KIND_LIN, m.n);
  CK(tmhip_field_upload(c, tmhip_field_even(m.f), host, pt.cnt[0]));
  if (pt.n > 1) CK(tmhip_field_upload(c, tmhip_field_odd(m.f), (const spinor *)host + VOLUME / 2, pt.cnt[1]));
}
// Other host threads may be reading the very field that is being brought up to date (an OpenMP loop over it: one thread's fault
// triggers the fetch, the others read on).  A page must therefore never be readable before its new contents are in place: opening
// the span, then copying, lets those threads read the old data for as long as the copy takes.  The new contents are assembled in a
// private mapping nobody else knows and moved over the program's pages with mremap(MREMAP_FIXED), which swaps the pages in one step:
// a reader sees a closed page (faults, waits for the lock, runs again) or the new one.  A page the field shares with other data is
// first taken out with MREMAP_DONTUNMAP (its address stays mapped, closed and empty), completed in private and moved back.
// [host, host + bytes) lies in the pages [lo, hi); src holds its new contents; the caller has already recorded the mirror's new
// state, so page_need() gives the protection every page ends up with.  false: this memory cannot be moved (not private anonymous
// memory, or a kernel before 5.7) and nothing was changed -- the caller falls back to open-then-copy.
bool g_install_ok = true;
bool take_page(uintptr_t page, char *to) {
  if (mprotect((void *)page, g_page, PROT_NONE)) return false;
  if (mremap((void *)page, g_page, g_page, MREMAP_MAYMOVE | MREMAP_FIXED | MREMAP_DONTUNMAP, to) != (void *)to) return false;
  return mprotect(to, g_page, PROT_READ | PROT_WRITE) == 0;
}
bool move_over(char *from, uintptr_t to, size_t len) {
  if (mprotect(from, len, prot_flags(page_need(to, g_reg)))) return false;
  return mremap(from, len, len, MREMAP_MAYMOVE | MREMAP_FIXED, (void *)to) == (void *)to;
}
bool install_pages(uintptr_t host, size_t bytes, uintptr_t lo, uintptr_t hi, const char *src) {
  if (!g_install_ok) return false;
  const size_t len = hi - lo;
  char *sc = (char *)mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (sc == MAP_FAILED) return false;
  const uintptr_t last = hi - g_page;
  const bool head = host > lo, tail = host + bytes < hi && (last != lo || !head);
  bool took_head = false;
  if (head) {
    if (!take_page(lo, sc)) { g_install_ok = false; munmap(sc, len); return false; }
    took_head = true;
  }
  if (tail && !take_page(last, sc + (last - lo))) {
    g_install_ok = false;
    if (took_head) { mprotect(sc, g_page, PROT_NONE); mremap(sc, g_page, g_page, MREMAP_MAYMOVE | MREMAP_FIXED, (void *)lo); munmap(sc + g_page, len - g_page); }
    else munmap(sc, len);
    return false;
  }
  memcpy(sc + (host - lo), src, bytes);
  // up to three pieces (the two shared pages are mappings of their own by now); each move is one step for every other thread
  bool ok = true;
  uintptr_t a = lo, b = hi;
  if (head) { ok = move_over(sc, lo, g_page) && ok; a = lo + g_page; }
  if (tail) { ok = move_over(sc + (last - lo), last, g_page) && ok; b = last; }
  if (a < b) ok = move_over(sc + (a - lo), a, b - a) && ok;
  if (!ok) die("lazy mode: mremap failed half-way while bringing a host array up to date");
  return true;
}

void download(tmhip_ctx *c, const void *host_user, Mirror &m) {
  const bool watched = m.prot != P_RW;                                  // lazy mode: the span is (partly) closed
  const bool staged = g_mode == TMLQCD_HIP_LAZY || watched;
  const void *host = staged ? bounce(m.bytes) : host_user;
  const Parts pt = parts_of(m.kind == KIND_LIN ? KIND_LIN : TMHIP_FIELD_EO, m.n);
  if (staged) {
    // straight into the page-locked bounce buffer: nothing of the context's own staging is touched, so the fault handler can do this
    // on a host thread while the master thread is inside another call
    if (m.kind != KIND_LIN) {
      CK(tmhip_field_download_range(c, m.f, const_cast<void *>(host), 0, nsites(m.kind)));
    } else {
      CK(tmhip_field_download_range(c, tmhip_field_even(m.f), const_cast<void *>(host), 0, pt.cnt[0]));
      if (pt.n > 1) CK(tmhip_field_download_range(c, tmhip_field_odd(m.f), (spinor *)const_cast<void *>(host) + VOLUME / 2, 0, pt.cnt[1]));
    }
  } else if (m.kind != KIND_LIN) {
    CK(tmhip_field_download(c, m.f, const_cast<void *>(host), nsites(m.kind)));
  } else {
    CK(tmhip_field_download(c, tmhip_field_even(m.f), const_cast<void *>(host), pt.cnt[0]));
    if (pt.n > 1) CK(tmhip_field_download(c, tmhip_field_odd(m.f), (spinor *)const_cast<void *>(host) + VOLUME / 2, pt.cnt[1]));
  }
  m.host_valid = true;
  if (!watched) { if (staged) memcpy(const_cast<void *>(host_user), host, m.bytes); return; }
  m.prot = g_mode == TMLQCD_HIP_LAZY ? P_RO : P_RW;                     // both copies current: watch for host stores
  std::fill(m.page_ok.begin(), m.page_ok.end(), 0); m.faults = 0;
  const uintptr_t lo = span_lo(host_user), hi = span_hi(host_user, m.bytes);
  if (install_pages((uintptr_t)host_user, m.bytes, lo, hi, (const char *)host)) return;
  mprotect((void *)lo, hi - lo, PROT_READ | PROT_WRITE);                // (memory that cannot be moved: open, copy, close)
  memcpy(const_cast<void *>(host_user), host, m.bytes);
  apply_prot(host_user, m, g_reg);
}
// the host array of a mirror is gone (freed and not handed out again: mincore says ENOMEM for an unmapped page): nothing to bring up to date
bool host_unmapped(const void *host, const Mirror &m) {
  if (!m.bytes) return false;
  unsigned char vec;
  const uintptr_t pg = span_lo((const char *)host + m.bytes / 2);
  return mincore((void *)pg, g_page, &vec) != 0 && errno == ENOMEM;
}
bool mapping_replaced(const void *host, const Mirror &m);
// a mirror is about to go away (or to stop being watched): bring the host up to date and give it its pages back
void release_host(tmhip_ctx *c, const void *host, Mirror &m) {
  // freed by the program (and possibly mapped again for something else, which a download would overwrite): there is no host copy
  // to bring up to date
  if (g_mode == TMLQCD_HIP_LAZY && m.prot != P_RW && (host_unmapped(host, m) || mapping_replaced(host, m))) {
    m.prot = P_RW; std::fill(m.page_ok.begin(), m.page_ok.end(), 0); m.dev_valid = false; m.host_valid = true;
    return;
  }
  if (m.f && m.dev_valid && !m.host_valid) download(c, host, m);
  if (m.prot != P_RW) set_prot(host, m, P_RW, g_reg);
}

// drop the least recently used mirrors that hold nothing the host does not have
void evict_if_crowded(tmhip_ctx *c, const void *keep) {
  static bool read_env = false;
  if (!read_env) { const char *e = getenv("TMLQCD_HIP_MAX_MIRRORS"); if (e && atoi(e) > 8) g_mirror_cap = (size_t)atoi(e); read_env = true; }
  RegLock lk;
  while (g_reg.size() > g_mirror_cap) {
    const void *victim = nullptr;
    unsigned long long oldest = ~0ull;
    for (auto &kv : g_reg)
      if (kv.first != keep && kv.second.host_valid && kv.second.last_use < oldest) { oldest = kv.second.last_use; victim = kv.first; }
    if (!victim) return;   // everything else is device-only data (resident mode): keep it
    release_host(c, victim, g_reg[victim]);
    if (g_reg[victim].f) tmhip_field_free(c, g_reg[victim].f);
    g_reg.erase(victim);
    rebuild_watch();
  }
}

// Lazy mode trusts a mirror across calls because it expects to SEE every host store (write-protected pages) and every host load of
// stale data (inaccessible pages).  That breaks when the program frees the array and gets the same address back: a large calloc is
// munmap'ed and mmap'ed again (solver/solver_field.c does this per solve in the solvers this library does not replace), the new
// pages are readable and writable, and nothing faults.  So before a watched mirror is trusted, one page of its span that this
// mirror alone protects is probed with system calls that fail with EFAULT instead of raising SIGSEGV:
//   P_NONE: write(2) FROM the page must fail;   P_RO: read(2) INTO the page (of the byte it already holds) must fail.
// If the probe succeeds the mapping is not the one this library protected: the host copy is the truth, the mirror starts over.
int g_probe_pipe[2] = {-1, -1};
bool mapping_replaced(const void *host, const Mirror &m) {
  if (m.prot == P_RW || !m.bytes) return false;
  const uintptr_t base = (uintptr_t)host, first = (base + g_page - 1) & ~(g_page - 1), last = (base + m.bytes) & ~(g_page - 1);   // interior pages [first, last)
  if (first >= last) return false;                                    // the field owns no whole page: its edge pages cannot have been unmapped alone
  uintptr_t pg = first + ((last - first) / g_page / 2) * g_page;      // a page in the middle
  if (m.prot == P_NONE) {                                             // ... that the host has not fetched meanwhile (those are read-only)
    const size_t i0 = (first - span_lo(host)) / g_page, i1 = (last - span_lo(host)) / g_page;
    size_t i = (pg - span_lo(host)) / g_page;
    if (i < m.page_ok.size() && m.page_ok[i]) {
      for (i = i0; i < i1 && i < m.page_ok.size() && m.page_ok[i]; i++) {}
      if (i >= i1 || i >= m.page_ok.size()) return false;             // every interior page already fetched: nothing left to tell by
      pg = span_lo(host) + i * g_page;
    }
  }
  if (g_probe_pipe[0] < 0 && pipe2(g_probe_pipe, O_NONBLOCK | O_CLOEXEC)) die("pipe() for the lazy mode's mapping probe failed");   // (non-blocking: a probe never waits)
  if (m.prot == P_NONE) {
    if (write(g_probe_pipe[1], (const void *)pg, 1) == 1) { char b; (void)!read(g_probe_pipe[0], &b, 1); return true; }
    return false;                                                     // EFAULT: still inaccessible, still ours
  }
  const char b = *(const volatile char *)pg;                          // P_RO: readable by construction
  if (write(g_probe_pipe[1], &b, 1) != 1) return false;               // (cannot probe: trust the mirror as before)
  if (read(g_probe_pipe[0], (void *)pg, 1) == 1) return true;         // the kernel could store into the page (the same byte): not write-protected any more
  char d; (void)!read(g_probe_pipe[0], &d, 1);                        // EFAULT: take the byte back out (if the kernel left it there)
  return false;
}

// Lazy mode watches an array by taking its pages away.  That is only sound for memory the program addresses and nobody else does:
//  * NOT inside a malloc arena -- the main one ("[heap]") or a thread's (a 64 MB-aligned mapping of at most 64 MB, read-write at the
//    bottom, PROT_NONE above: glibc's HEAP_MAX_SIZE): such pages also hold the allocator's chunk headers, free() / malloc() touch them
//    while they hold the arena's lock, and a fault taken there cannot be served (the handler's own callees allocate).  glibc serves a
//    request from an arena whenever a free chunk fits, whatever M_MMAP_THRESHOLD says (a 200 KB numpy array in a process that has
//    freed a few MB) -- which is why this library does NOT touch the program's malloc settings any more (it pinned the mmap threshold
//    until round 3; blocks above glibc's 32 MB ceiling of that threshold -- tmLQCD's fields at production sizes -- are mappings of
//    their own in any case);
//  * private and anonymous ("rw-p", no file): the handler swaps pages in with mremap(MREMAP_FIXED), which would silently turn a
//    MAP_SHARED / file-backed / hugetlb / SysV segment into private memory.
// Anything else is simply not watched: it is copied on every call, as in the coherent mode.  /proc/self/maps is read when a mirror is
// made (or its array was re-mapped), in entry-point context.
uintptr_t g_heap_lo = 0;   // start of the "[heap]" mapping (the initial program break: it never moves), 1 = there is none
bool below_program_break(const void *host) { return g_heap_lo > 1 && (uintptr_t)host >= g_heap_lo && (uintptr_t)host < (uintptr_t)sbrk(0); }
const char *unwatchable(const void *host, size_t bytes) {
  const uintptr_t a = (uintptr_t)host, b = a + bytes;
  FILE *fp = fopen("/proc/self/maps", "r");
  if (!fp) return "cannot read /proc/self/maps";
  // The array may lie in SEVERAL lines: this library's own mprotect calls (a neighbouring field's read-only or closed pages) split the
  // block's mapping by protection.  So the contiguous run of private anonymous lines around it is taken as a whole, whatever their
  // permissions are at the moment; it must cover [a, b).
  const char *why = nullptr;
  char line[512];
  bool in_run = false, last_none = false;
  unsigned long first_lo = 0, covered = 0;
  const unsigned long ARENA = (unsigned long)64 << 20;     // glibc's HEAP_MAX_SIZE
  while (fgets(line, sizeof(line), fp)) {
    unsigned long lo = 0, hi = 0, off = 0, ino = 0; char perm[8] = "", dev[16] = ""; int consumed = 0;
    if (sscanf(line, "%lx-%lx %7s %lx %15s %lu %n", &lo, &hi, perm, &off, dev, &ino, &consumed) < 6) continue;
    const char *name = line + consumed;
    const bool heap = strstr(name, "[heap]") != nullptr;
    if (!g_heap_lo && heap) g_heap_lo = lo;
    const bool private_anon = perm[3] == 'p' && ino == 0 && (!name[0] || name[0] == '\n');
    if (!in_run) {
      if (a < lo || a >= hi) continue;
      in_run = true; first_lo = lo; covered = hi;
      if (heap) { why = "inside the malloc heap"; break; }
      if (perm[3] != 'p') { why = "a shared mapping"; break; }
      if (!private_anon) { why = "a file-backed or named mapping"; break; }
      last_none = !strncmp(perm, "---", 3);
      continue;
    }
    if (lo != covered || !private_anon) {       // the run ends here
      if (covered < b) why = lo != covered ? "not mapped contiguously" : "spans mappings of different kinds";
      break;
    }
    covered = hi; last_none = !strncmp(perm, "---", 3);
    if (covered - first_lo > ARENA) break;        // (longer than any arena: enough is known)
  }
  fclose(fp);
  if (!g_heap_lo) g_heap_lo = 1;   // (the heap line comes before any mmap region: if it was not seen up to the array's line, there is none)
  if (!in_run) return "not mapped";
  if (why) return why;
  if (covered < b) return "not mapped contiguously";
  // a thread's arena: 64 MB-aligned, read-write at the bottom, its PROT_NONE reserve up to the 64 MB boundary
  if (first_lo % ARENA == 0 && covered == first_lo + ARENA && last_none) return "inside a thread's malloc arena";
  return nullptr;
}

Mirror &mirror(tmhip_ctx *c, const void *host, int kind, int n = 0) {
  RegLock lk;
  const size_t bytes = (size_t)(kind == KIND_LIN ? n : nsites(kind)) * sizeof(spinor);
  const bool known = g_reg.find(host) != g_reg.end();
  bool remapped = false;
  if (!known) evict_if_crowded(c, host);
  if (g_mode == TMLQCD_HIP_LAZY) {
    // One device mirror per host byte, checked on EVERY call: an array the program now addresses from another base (the halves of
    // a full field, a block inside a field) or with another extent at the SAME base (the even half at X becomes the full field at
    // X, a prefix grows) must not leave a second, independently valid copy of some of its bytes in HBM -- e.g. Hopping_Matrix into
    // g_spinor_field[k] and [k+1], then D_psi or square_norm(., VOLUME) on the pair.
    std::vector<const void *> overlap;
    for (auto &kv : g_reg)
      if (kv.first != host && (uintptr_t)kv.first < (uintptr_t)host + bytes && (uintptr_t)host < (uintptr_t)kv.first + kv.second.bytes) overlap.push_back(kv.first);
    for (const void *o : overlap) {
      release_host(c, o, g_reg[o]);
      if (g_reg[o].f) tmhip_field_free(c, g_reg[o].f);
      g_reg.erase(o);
    }
    if (!overlap.empty()) rebuild_watch();
    if (known && mapping_replaced(host, g_reg[host])) {   // freed and re-allocated at the same address: the host copy is the truth
      remapped = true;
      Mirror &old = g_reg[host];
      old.dev_valid = false; old.host_valid = true; old.prot = P_RW; std::fill(old.page_ok.begin(), old.page_ok.end(), 0); old.faults = 0;
    }
  }
  // (the main heap may have grown over a recycled address since the array was classified: one comparison with the program break, no file)
  const bool reclassify = g_mode == TMLQCD_HIP_LAZY && known && g_reg[host].prot == P_RW && !g_reg[host].nowatch && below_program_break(host);
  Mirror &m = g_reg[host];
  if (m.f && (m.kind != kind || (kind == KIND_LIN && m.n != n))) {   // same host buffer re-used with another shape (or another prefix length)
    release_host(c, host, m);
    tmhip_field_free(c, m.f);
    m = Mirror();
  }
  bool fresh = false;
  if (!m.f) {
    CK(tmhip_field_alloc(c, kind == KIND_LIN ? TMHIP_FIELD_FULL : kind, &m.f));
    m.kind = kind; m.n = n; m.dev_valid = false; m.host_valid = true; m.bytes = bytes; m.prot = P_RW;
    fresh = true;
  }
  if (g_mode == TMLQCD_HIP_LAZY && m.prot == P_RW && (fresh || reclassify || remapped || !m.classified)) {
    // decided while the array is unwatched, and everything the fault handler will need for it is made NOW
    const char *why = unwatchable(host, bytes);
    static const bool force = getenv("TMLQCD_HIP_LAZY_FORCE_WATCH") != nullptr;     // test hook: watch it anyway, a fault on it must end loudly
    m.nowatch = why != nullptr && !force;
    m.unsafe = why != nullptr && force;
    m.classified = true;
    static const bool dbg = getenv("TMLQCD_HIP_LAZY_DEBUG") != nullptr;
    if (why && dbg) fprintf(stderr, "[tmlqcd_dropin] lazy mode: the array at %p (%zu bytes) is %s: %s\n", host, bytes, force ? "WATCHED ALTHOUGH IT SHOULD NOT BE (test hook)" : "not watched, copied per call", why);
    if (!m.nowatch) {
      prepare_handler_buffers(bytes);
      m.page_ok.assign((span_hi(host, bytes) - span_lo(host)) / g_page, 0);
    }
  }
  if (!known || fresh) rebuild_watch();
  m.last_use = ++g_tick;   // after the reset above: a mirror in use by the current call must never be the eviction victim of its sibling
  return m;
}

}  // namespace

tmhip_field *in(tmhip_ctx *c, const void *host, int kind, int n) {
  RegLock lk;   // a mirror's state changes under the lock too: the fault handler reads it on other threads
  Mirror &m = mirror(c, host, kind, n);
  const bool copy_always = g_mode == TMLQCD_HIP_COHERENT || (g_mode == TMLQCD_HIP_LAZY && m.nowatch);
  if (copy_always || !m.dev_valid) {
    if (!(m.dev_valid && !m.host_valid))   // never overwrite newer device data with a stale host copy
      upload(c, host, m);
    m.dev_valid = true;
  }
  if (g_mode == TMLQCD_HIP_LAZY && !m.nowatch && m.host_valid && m.prot == P_RW) set_prot(host, m, P_RO, g_reg);   // the mirror stays good until the host stores to the array
  return m.f;
}

tmhip_field *out(tmhip_ctx *c, const void *host, int kind, int n) { return mirror(c, host, kind, n).f; }

void done(tmhip_ctx *c, const void *host) {
  RegLock lk;
  Mirror &m = g_reg[host];
  m.dev_valid = true; m.host_valid = false;
  if (g_mode == TMLQCD_HIP_COHERENT || (g_mode == TMLQCD_HIP_LAZY && m.nowatch)) {
    download(c, host, m);
    m.dev_valid = false;   // coherent mode: the host copy is the truth (it may be rewritten or its address recycled)
  } else if (g_mode == TMLQCD_HIP_LAZY) {
    set_prot(host, m, P_NONE, g_reg);   // the host's next load from the array faults and fetches what it needs
  }
}

namespace {

// SIGSEGV on a protected page of a mirrored host array (lazy mode); anything else goes to the handler that was there before.
//
// What this handler may do, and why it cannot hang (round-3 review, item 5; the hang of gpurun_out/r03_mp_*.log was a fault taken
// inside malloc, on a watched page of the malloc heap, with the handler's callees then waiting for the allocator's lock):
//  * It allocates nothing itself: the table it walks is a fixed array (g_watch), every mirror's page map was sized when the mirror
//    was made, its page-locked buffers (staging buffer of the largest watched array, the 64-spinor page buffer) exist before an array is
//    first watched (prepare_handler_buffers).  A request beyond them ends the program with a message (handler_die), never a retry.
//  * It DOES enter the HIP runtime: tmhip_field_download_range = one kernel launch that writes into page-locked memory + a stream
//    synchronisation.  The runtime takes its own locks there and may allocate.  That is safe because the INTERRUPTED thread can hold
//    neither a runtime lock nor an allocator lock at the moment of the fault:
//      - the only code that ever touches a watched page is the program's own loads and stores and this library's host -> bounce
//        memcpy of an upload (which holds only the registry lock, recursive for its owner).  The HIP runtime never sees a pointer
//        into the program's arrays in this mode -- every transfer goes through the page-locked bounce buffers -- so no fault can be
//        raised from inside the runtime (the "bounce-buffer argument");
//      - no watched page holds allocator state: arrays inside a malloc arena, main or per-thread, are not watched (unwatchable());
//        an mmap'ed block's own header lies in front of the user pointer, and free() of such a block takes no arena lock.
//    ANOTHER thread may be inside the runtime or the allocator (the master thread in an entry point while an OpenMP worker faults):
//    then this handler waits for an ordinary lock whose holder is running -- a delay, not a cycle; the registry lock is the only one
//    held across, and its holder never waits for a faulting thread.
//  * TMLQCD_HIP_LAZY_FORCE_WATCH (test hook) watches an unwatchable array anyway; a fault on one of its pages is answered with a
//    message and _exit(1) before anything else is called (tests/test_gpu_lazy.py).
void lazy_fault(int sig, siginfo_t *si, void *uctx) {
  const uintptr_t addr = (uintptr_t)si->si_addr, page = addr & ~(g_page - 1);
  bool ours = false;
  // Host threads (an OpenMP loop over a stale field) may fault at the same time, and the master thread may be inside an entry point
  // that changes the registry: one at a time in here, under the registry's lock.  A fault of the thread that already is in the
  // handler would be a bug of this handler: let it crash instead of recursing.
  const bool nested = in_handler_here();
  static const bool trace = getenv("TMLQCD_HIP_LAZY_DEBUG") != nullptr && atoi(getenv("TMLQCD_HIP_LAZY_DEBUG")) > 1;
  if (trace) {   // (debugging aid, TMLQCD_HIP_LAZY_DEBUG=2: names the object the faulting instruction lives in -- dladdr is not async-signal-safe)
    Dl_info di; memset(&di, 0, sizeof(di));
    void *ip = (void *)((ucontext_t *)uctx)->uc_mcontext.gregs[REG_RIP];
    dladdr(ip, &di);
    char m[384]; const int n = snprintf(m, sizeof(m), "[lazy] fault %p %s enter, instruction %p in %s (%s)\n", si->si_addr, (((ucontext_t *)uctx)->uc_mcontext.gregs[REG_ERR] & 2) ? "store" : "load", ip, di.dli_fname ? di.dli_fname : "?", di.dli_sname ? di.dli_sname : "?"); (void)!write(2, m, (size_t)n);
  }
  if (live_ctx() && si->si_code == SEGV_ACCERR && !nested) {
    RegLock lk;
    g_handler_thread.store((uintptr_t)pthread_self(), std::memory_order_relaxed);
    const bool store = (((ucontext_t *)uctx)->uc_mcontext.gregs[REG_ERR] & 2) != 0;
    for (int wk = 0; wk < g_nwatch; wk++) {
      Mirror &m = *g_watch[wk].m;
      const void *host = g_watch[wk].host;
      if (!m.bytes || page < span_lo(host) || page >= span_hi(host, m.bytes)) continue;
      ours = true;                                   // (also when another thread has opened the page in the meantime: just run again)
      if (m.prot == P_RW) continue;
      if (m.unsafe) handler_die("[tmlqcd_dropin] fatal: lazy mode: fault on a watched page of an array that must not be watched (malloc arena / shared mapping; TMLQCD_HIP_LAZY_FORCE_WATCH): ending instead of risking a deadlock\n");
      if (store) {
        g_lazy_stats[3]++;                                   // the host is about to change the array: its copy becomes the only good one
        if (!m.host_valid) download(live_ctx(), host, m);
        m.dev_valid = false;
        set_prot(host, m, P_RW, g_reg);
      } else if (m.prot == P_NONE) {
        const size_t idx = (page - span_lo(host)) / g_page;
        if (m.page_ok[idx]) continue;                // (the page was closed by a neighbour's wish only)
        if (m.kind != TMHIP_FIELD_EO || ++m.faults > LAZY_PAGE_FAULTS) {
          g_lazy_stats[2]++;
          download(live_ctx(), host, m);                  // the host reads on: fetch the rest in one go (both copies stay current, P_RO)
        } else {
          const uintptr_t base = (uintptr_t)host, lo = page > base ? page : base, hi = page + g_page < base + m.bytes ? page + g_page : base + m.bytes;
          const int s0 = (int)((lo - base) / sizeof(spinor)), s1 = (int)((hi - base + sizeof(spinor) - 1) / sizeof(spinor));
          void *tmp = g_page_tmp;                     // page-locked, made when the first array was watched (prepare_handler_buffers)
          if (!tmp || s1 - s0 > 64) handler_die("[tmlqcd_dropin] fatal: lazy mode: no page buffer for a page-wise fetch\n");
          if (tmhip_field_download_range(live_ctx(), m.f, tmp, s0, s1 - s0)) handler_die("[tmlqcd_dropin] fatal: lazy synchronisation of a page failed\n");
          m.page_ok[idx] = 1;
          const char *from = (const char *)tmp + (lo - (base + (size_t)s0 * sizeof(spinor)));
          if (!install_pages(lo, hi - lo, page, page + g_page, from)) {
            mprotect((void *)page, g_page, PROT_READ | PROT_WRITE);
            memcpy((void *)lo, from, hi - lo);
          }
          g_lazy_stats[1]++;
        }
      }
    }
    if (ours) { g_lazy_stats[0]++; mprotect((void *)page, g_page, prot_flags(page_need(page, g_reg))); }
    g_handler_thread.store(0, std::memory_order_relaxed);
  }
  if (trace) { char m[64]; const int n = snprintf(m, sizeof(m), "[lazy] fault %p leave ours=%d\n", si->si_addr, (int)ours); (void)!write(2, m, (size_t)n); }
  if (ours) return;                                  // the faulting instruction runs again
  {
    // TMLQCD_HIP_LAZY_DEBUG=1: say what is being passed on (the program's own crash, or a bug of this handler) before the next handler sees it
    static const bool dbg = getenv("TMLQCD_HIP_LAZY_DEBUG") != nullptr;
    if (dbg) {
      char msg[256];
      const int n = snprintf(msg, sizeof(msg), "[tmlqcd_dropin] SIGSEGV at %p (si_code %d, %s) is not on a watched page of %zu mirrors%s: passed on\n", si->si_addr,
                             si->si_code, (((ucontext_t *)uctx)->uc_mcontext.gregs[REG_ERR] & 2) ? "store" : "load", g_reg.size(), nested ? ", raised inside this handler" : "");
      if (n > 0) (void)!write(2, msg, (size_t)n);
    }
  }
  if (g_old_segv.sa_flags & SA_SIGINFO) { if (g_old_segv.sa_sigaction) { g_old_segv.sa_sigaction(sig, si, uctx); return; } }
  else if (g_old_segv.sa_handler != SIG_DFL && g_old_segv.sa_handler != SIG_IGN) { g_old_segv.sa_handler(sig); return; }
  signal(SIGSEGV, SIG_DFL);                          // not ours, nobody else's: die the ordinary way when the instruction faults again
}
void install_lazy_handler() {
  if (g_handler_installed) return;
  g_page = (uintptr_t)sysconf(_SC_PAGESIZE);
  // (the program's malloc settings are left alone: arrays that cannot be watched are recognised one by one, unwatchable())
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = lazy_fault;
  sa.sa_flags = SA_SIGINFO | SA_NODEFER;
  sigemptyset(&sa.sa_mask);
  if (sigaction(SIGSEGV, &sa, &g_old_segv)) die("cannot install the SIGSEGV handler of the lazy residency mode");
  g_handler_installed = true;
}

}  // namespace

// ------------------------------------------------------------------ what dropin.cpp asks of this module (dropin_internal.h)
int residency_mode() { return g_mode; }
void residency_from_env() {
  const char *r = getenv("TMLQCD_HIP_RESIDENCY");       // unmodified executables: TMLQCD_HIP_RESIDENCY=lazy ./benchmark
  if (r && !strcmp(r, "lazy") && g_mode == TMLQCD_HIP_COHERENT) { install_lazy_handler(); g_mode = TMLQCD_HIP_LAZY; }
  else if (r && !strcmp(r, "resident") && g_mode == TMLQCD_HIP_COHERENT) g_mode = TMLQCD_HIP_RESIDENT;
}
void release_all_mirrors(tmhip_ctx *c) {
  RegLock lk;
  tmlqcd_hip_sync_all_to_host();
  for (auto &kv : g_reg) { if (kv.second.prot != P_RW) set_prot(kv.first, kv.second, P_RW, g_reg); if (kv.second.f) tmhip_field_free(c, kv.second.f); }
  g_reg.clear();
  g_nwatch = 0;
  for (int k = 0; k < 2; k++) if (g_bounce[k]) { tmhip_pinned_free(g_bounce[k]); g_bounce[k] = nullptr; g_bounce_bytes[k] = 0; }
  if (g_page_tmp) { tmhip_pinned_free(g_page_tmp); g_page_tmp = nullptr; }
}
CoherentScope::CoherentScope() : saved(g_mode) { tmlqcd_hip_set_residency(TMLQCD_HIP_COHERENT); }
CoherentScope::~CoherentScope() { g_mode = saved; }
static int g_bench_saved = TMLQCD_HIP_COHERENT;
void bench_begin() {
  reg_lock();   // given back by bench_finish
  g_bench_saved = g_mode;
  g_mode = TMLQCD_HIP_RESIDENT;
}
void bench_finish(tmhip_ctx *c, spinor *f1, spinor *f2) {
  g_reg[f1].dev_valid = true; g_reg[f1].host_valid = false;
  g_reg[f2].dev_valid = true; g_reg[f2].host_valid = false;
  g_mode = g_bench_saved;
  if (g_mode == TMLQCD_HIP_COHERENT) { tmlqcd_hip_sync_to_host(f1); tmlqcd_hip_sync_to_host(f2); }
  if (g_mode == TMLQCD_HIP_LAZY)
    for (spinor *f : {f1, f2}) {
      Mirror &m = g_reg[f];
      if (m.nowatch) { download(c, f, m); m.dev_valid = false; }   // (an array inside the malloc heap: copied, never watched)
      else set_prot(f, m, P_NONE, g_reg);
    }
  reg_unlock();
}

extern "C" {

// ------------------------------------------------------------------ residency control
void tmlqcd_hip_lazy_stats(unsigned long out[4]) { for (int k = 0; k < 4; k++) out[k] = g_lazy_stats[k]; }
void tmlqcd_hip_set_residency(int mode) {
  if (mode != TMLQCD_HIP_COHERENT && mode != TMLQCD_HIP_RESIDENT && mode != TMLQCD_HIP_LAZY) die("tmlqcd_hip_set_residency: unknown mode");
  RegLock lk;
  if (mode == TMLQCD_HIP_COHERENT && g_mode == TMLQCD_HIP_RESIDENT) tmlqcd_hip_sync_all_to_host();
  if (g_mode == TMLQCD_HIP_LAZY && mode != TMLQCD_HIP_LAZY)        // leaving lazy mode: every host array current and unwatched again
    for (auto &kv : g_reg) release_host(ctx(), kv.first, kv.second);
  if (mode == TMLQCD_HIP_LAZY) install_lazy_handler();
  // whenever the host copy is current it is authoritative: a mirror left over from an earlier call may belong to a
  // host array that has since been rewritten, or to a freed one whose address was recycled
  for (auto &kv : g_reg) if (kv.second.host_valid) kv.second.dev_valid = false;
  g_mode = mode;
}
void tmlqcd_hip_sync_to_host(spinor *field) {
  RegLock lk;
  auto it = g_reg.find(field);
  if (it == g_reg.end() || !it->second.f) return;
  if (it->second.dev_valid && !it->second.host_valid) download(ctx(), field, it->second);
}
void tmlqcd_hip_sync_all_to_host(void) {
  RegLock lk;
  for (auto &kv : g_reg)
    if (kv.second.f && kv.second.dev_valid && !kv.second.host_valid) download(ctx(), kv.first, kv.second);
}
void tmlqcd_hip_host_modified(spinor *field) {
  RegLock lk;
  auto it = g_reg.find(field);
  if (it != g_reg.end()) {
    it->second.dev_valid = false; it->second.host_valid = true;
    if (it->second.prot != P_RW) set_prot(field, it->second, P_RW, g_reg);
  }
}
void tmlqcd_hip_forget(spinor *field) {
  RegLock lk;
  auto it = g_reg.find(field);
  if (it == g_reg.end()) return;
  if (it->second.prot != P_RW) { it->second.host_valid = true; set_prot(field, it->second, P_RW, g_reg); }   // (the array is being freed: nothing to fetch)
  if (it->second.f) tmhip_field_free(live_ctx(), it->second.f);
  g_reg.erase(it);
  rebuild_watch();
}
void tmlqcd_hip_set_max_mirrors(int n) { if (n >= 8) g_mirror_cap = (size_t)n; }

}  // extern "C"
