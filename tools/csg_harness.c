/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_csg.py together with the reference's own solver/chrono_guess.c,
 * solver/lu_solve.c and the complex linalg files oracle/_ref/libtmref.so does not define (compiled in place into a temporary
 * directory) and libtmref.so, which provides the operators, cg_her, the real linalg set, the geometry and the globals.
 *
 * Glue only: the debug switch the reference's chrono_guess reads, and an entry that runs LUSolve on caller-owned arrays. */
#include <complex.h>

extern int g_debug_level;
void tmcsg_set_debug(int level) { g_debug_level = level; }

void LUSolve(const int Nvec, _Complex double *M, const int ldM, _Complex double *b);
void tmcsg_lusolve(int n, double *M, int ld, double *b) { LUSolve(n, (_Complex double *)M, ld, (_Complex double *)b); }
