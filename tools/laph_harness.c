/* TEST INFRASTRUCTURE ONLY: linked by tools/make_golden_laph.py together with the reference's own jacobi.c, geometry_eo.c and
 * init/init_geometry_indices.c, compiled in place with -DWITHLAPH into a temporary directory.  This file instantiates the
 * reference's globals through its own mechanism (global.h: INIT_GLOBALS), sets the lattice, lets the reference's geometry() fill
 * g_iup3d / g_idn3d and hands the reference's Jacobi() a gauge field and a colour vector.  No reference algorithm is restated here. */
#define INIT_GLOBALS
#include <stdlib.h>
#include <string.h>
#include "global.h"
#include "su3.h"
#include "geometry_eo.h"
#include "init/init_geometry_indices.h"
#include "jacobi.h"

static su3 *links = NULL;

int tmlaph_init(int T_, int LX_, int LY_, int LZ_) {
  int i;
  g_nproc = 1; g_proc_id = 0; g_nproc_x = g_nproc_y = g_nproc_z = g_nproc_t = 1;
  g_cart_id = 0; g_stdio_proc = 0;
  g_proc_coords[0] = g_proc_coords[1] = g_proc_coords[2] = g_proc_coords[3] = 0;
  T_global = T_; T = T_; L = LX_; LX = LX_; LY = LY_; LZ = LZ_;
  VOLUME = T * LX * LY * LZ; SPACEVOLUME = VOLUME / T;
  RAND = 0; EDGES = 0; VOLUMEPLUSRAND = VOLUME; SPACERAND = 0;
  N_PROC_T = N_PROC_X = N_PROC_Y = N_PROC_Z = 1;
  g_dbw2rand = 0; lowmem_flag = 0; g_debug_level = 0;
  if (init_geometry_indices(VOLUMEPLUSRAND + g_dbw2rand) != 0) return 1;
  links = calloc((size_t)4 * VOLUME, sizeof(su3));
  g_gauge_field = calloc(VOLUME, sizeof(su3 *));
  if (!links || !g_gauge_field) return 2;
  for (i = 0; i < VOLUME; i++) g_gauge_field[i] = links + 4 * (size_t)i;
  geometry();
  return 0;
}
/* su3 [VOLUME][4], the lexicographic field */
void tmlaph_set_gauge(const double *g) { memcpy(links, g, (size_t)4 * VOLUME * sizeof(su3)); }
int tmlaph_spacevolume(void) { return SPACEVOLUME; }
/* l, k: su3_vector [SPACEVOLUME] */
void tmlaph_jacobi(double *l, double *k, int t) { Jacobi((su3_vector *)l, (su3_vector *)k, t); }
/* g_iup3d / g_idn3d as the reference's geometry() left them: int [SPACEVOLUME][4] each */
void tmlaph_neighbours(int *up, int *dn) {
  int i, mu;
  for (i = 0; i < SPACEVOLUME; i++)
    for (mu = 0; mu < 4; mu++) { up[4 * i + mu] = g_iup3d[i][mu]; dn[4 * i + mu] = g_idn3d[i][mu]; }
}
