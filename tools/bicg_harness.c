/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_bicg.py together with the reference's own solver/bicgstab_complex.c and the
 * complex linalg files oracle/_ref/libtmref.so does not define (compiled in place into a temporary directory) and libtmref.so, which
 * provides the operators, the solver fields, the real linalg set, the geometry and the globals.
 *
 * Glue only: the debug switch (at level 3 the reference's bicgstab_complex prints "i err" at the top of every iteration, which is
 * how the generator learns its recursive residual) and a flush of the C stream the lines go to. */
#include <stdio.h>

extern int g_debug_level;
void tmbicg_set_debug(int level) { g_debug_level = level; }
void tmbicg_flush(void) { fflush(stdout); }
