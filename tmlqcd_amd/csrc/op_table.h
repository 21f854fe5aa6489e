// The operators the solvers know by id (TMHIP_OP_*, TMHIP_ND_OP_* of include/tmlqcd_hip.h): ONE list, read by the core library
// (hipcc) and by the drop-in (g++), so no HIP in here.  Everything that asks "what is operator id n, what fields does it act on, what
// must the context hold, which solver takes it" asks a row of this list:
//   core    tmhip_apply_op / tmhip_apply_nd_op expand the rows with tmhip_<name>; tmhip_op_check / tmhip_nd_op_check (ops.hip) are the
//           one refusal every solver entry point starts with
//   drop-in dev_op_of / dev_nd_op_of (dropin.cpp) expand them with &<name>
// Adding an operator: its function, its enum value in the public header, one row here (and its name in tmlqcd_amd/hip.py).
#ifndef TMHIP_OP_TABLE_H
#define TMHIP_OP_TABLE_H
#include "../../include/tmlqcd_hip.h"

// the solver column: who takes the row.  The mixed solvers have no bit: they take exactly the rows with an fp32 twin.
enum { TMHIP_S_CG = 1      /* cg_her (both forms), chrono_guess */,
       TMHIP_S_MMS = 2     /* cg_mms_tm */,
       TMHIP_S_RATCOR = 4  /* apply_Z, ratcor_* */,
       TMHIP_S_BICG = 8    /* bicgstab_complex */,
       TMHIP_S_ND = 16     /* the doublet solvers, Ptilde_ndpsi, apply_Z_nd, ndratcor_* */,
       TMHIP_S_MIXED = 32  /* mixed_cg_her, rg_mixed_cg_her: asked through the fp32 column */,
       TMHIP_S_EIG = 64    /* eigenvalues: the Hermitian positive single-flavour rows (the doublet call takes the TMHIP_S_ND rows) */ };
// the clover column: what the context must hold.  TERM: sw and sw_inv valid (doublet rows: sw and sw_inv_nd); TERM_MINUS_MU: with
// mu != 0 additionally the -mu set of sw_inv
enum { TMHIP_SW_NONE = 0, TMHIP_SW_TERM = 1, TMHIP_SW_TERM_MINUS_MU = 2 };

//  id suffix       reference function   fields  clover          fp32  solvers
#define TMHIP_OP_TABLE(X)                                                                                 \
  X(QTM_PM,         Qtm_pm_psi,          EO,     NONE,           1,    TMHIP_S_CG | TMHIP_S_MMS | TMHIP_S_RATCOR | TMHIP_S_EIG) \
  X(QTM_PLUS,       Qtm_plus_psi,        EO,     NONE,           0,    TMHIP_S_CG | TMHIP_S_BICG)         \
  X(QTM_MINUS,      Qtm_minus_psi,       EO,     NONE,           0,    TMHIP_S_CG | TMHIP_S_BICG)         \
  X(MTM_PLUS,       Mtm_plus_psi,        EO,     NONE,           0,    TMHIP_S_CG | TMHIP_S_BICG)         \
  X(MTM_MINUS,      Mtm_minus_psi,       EO,     NONE,           0,    TMHIP_S_CG | TMHIP_S_BICG)         \
  X(QSW_PM,         Qsw_pm_psi,          EO,     TERM,           1,    TMHIP_S_CG | TMHIP_S_MMS | TMHIP_S_RATCOR | TMHIP_S_EIG) \
  X(Q_PM_FULL,      Q_pm_psi,            FULL,   NONE,           0,    TMHIP_S_MMS | TMHIP_S_EIG)         \
  X(MTM_PLUS_SYM,   Mtm_plus_sym_psi,    EO,     NONE,           0,    TMHIP_S_BICG)                      \
  X(MTM_MINUS_SYM,  Mtm_minus_sym_psi,   EO,     NONE,           0,    TMHIP_S_BICG)                      \
  X(QSW_PLUS,       Qsw_plus_psi,        EO,     TERM,           0,    TMHIP_S_BICG)                      \
  X(QSW_MINUS,      Qsw_minus_psi,       EO,     TERM_MINUS_MU,  0,    TMHIP_S_BICG)                      \
  X(MSW_PLUS,       Msw_plus_psi,        EO,     TERM,           0,    TMHIP_S_BICG)                      \
  X(D_PSI,          D_psi,               FULL,   NONE,           0,    TMHIP_S_BICG)
#define TMHIP_ND_OP_TABLE(X)                                                                              \
  X(QTM_PM,         Qtm_pm_ndpsi,        EO,     NONE,           1,    TMHIP_S_ND)                        \
  X(QSW_PM,         Qsw_pm_ndpsi,        EO,     TERM,           0,    TMHIP_S_ND)

struct tmhip_op_row { int id; const char *name; int kind, clover, fp32, solvers; };
#define TMHIP_OP_ROW(ID, NAME, KIND, SW, FP32, SOLVERS) {TMHIP_OP_##ID, #NAME, TMHIP_FIELD_##KIND, TMHIP_SW_##SW, FP32, SOLVERS},
#define TMHIP_ND_OP_ROW(ID, NAME, KIND, SW, FP32, SOLVERS) {TMHIP_ND_OP_##ID, #NAME, TMHIP_FIELD_##KIND, TMHIP_SW_##SW, FP32, SOLVERS},

// the row of an id, nullptr for an id outside the list
static inline const tmhip_op_row *tmhip_row_in(const tmhip_op_row *rows, int n, int op) {
  for (int i = 0; i < n; i++) if (rows[i].id == op) return &rows[i];
  return nullptr;
}
static inline const tmhip_op_row *tmhip_op_row_of(int op) {
  static const tmhip_op_row rows[] = {TMHIP_OP_TABLE(TMHIP_OP_ROW)};
  return tmhip_row_in(rows, (int)(sizeof(rows) / sizeof(rows[0])), op);
}
static inline const tmhip_op_row *tmhip_nd_op_row_of(int op) {
  static const tmhip_op_row rows[] = {TMHIP_ND_OP_TABLE(TMHIP_ND_OP_ROW)};
  return tmhip_row_in(rows, (int)(sizeof(rows) / sizeof(rows[0])), op);
}
static inline bool tmhip_op_taken(const tmhip_op_row *r, int solver) { return solver == TMHIP_S_MIXED ? r->fp32 != 0 : (r->solvers & solver) != 0; }

#endif
