// The operator table at work (op_table.h): the one dispatcher by id and the one refusal every solver entry point starts with.
// Host code only.
#include "tmhip_internal.h"

int tmhip_apply_op(tmhip_ctx *ctx, int op, tmhip_field *l, tmhip_field *k) {
  switch (op) {
#define X(ID, NAME, KIND, SW, FP32, SOLVERS) case TMHIP_OP_##ID: return tmhip_##NAME(ctx, l, k);
    TMHIP_OP_TABLE(X)
#undef X
  }
  TMHIP_FAIL("apply_op: %d is no operator id", op);
}

int tmhip_apply_nd_op(tmhip_ctx *ctx, int op, tmhip_field *l_s, tmhip_field *l_c, tmhip_field *k_s, tmhip_field *k_c) {
  switch (op) {
#define X(ID, NAME, KIND, SW, FP32, SOLVERS) case TMHIP_ND_OP_##ID: return tmhip_##NAME(ctx, l_s, l_c, k_s, k_c);
    TMHIP_ND_OP_TABLE(X)
#undef X
  }
  TMHIP_FAIL("apply_nd_op: %d is no doublet operator id", op);
}

int tmhip_op_check(tmhip_ctx *ctx, const char *who, int solver, int op, int kind) {
  const tmhip_op_row *r = tmhip_op_row_of(op);
  if (!r) TMHIP_FAIL("%s: %d is no operator id (TMHIP_OP_*)", who, op);
  if (!tmhip_op_taken(r, solver)) TMHIP_FAIL("%s does not take %s (operator id %d)", who, r->name, op);
  if (kind != r->kind) TMHIP_FAIL("%s: %s acts on %s fields", who, r->name, r->kind == TMHIP_FIELD_FULL ? "FULL" : "one-parity (EO)");
  if (r->clover != TMHIP_SW_NONE && !ctx->clover_set)
    TMHIP_FAIL("%s: %s without a valid clover term (tmhip_set_clover, or tmhip_sw_term and tmhip_sw_invert)", who, r->name);
  if (r->clover == TMHIP_SW_TERM_MINUS_MU && fabs(ctx->mu) > 0 && ctx->sw_inv_sets < 2)
    TMHIP_FAIL("%s: %s with mu != 0 needs the -mu set of sw_inv (sw_invert with the current mu)", who, r->name);
  return 0;
}

int tmhip_ndsw_ready(tmhip_ctx *ctx, const char *who, bool need_inv) {
  if (!ctx->sw_set) TMHIP_FAIL("%s called before tmhip_sw_term / tmhip_set_clover", who);
  if (need_inv && !ctx->clover_nd_set) TMHIP_FAIL("%s: sw_inv_nd is not valid: call tmhip_sw_invert_nd on the current clover term", who);
  return 0;
}

int tmhip_nd_op_check(tmhip_ctx *ctx, const char *who, int op, int solver) {
  const tmhip_op_row *r = tmhip_nd_op_row_of(op);
  if (!r) TMHIP_FAIL("%s: %d is no doublet operator id (TMHIP_ND_OP_*)", who, op);
  if (!tmhip_op_taken(r, solver)) TMHIP_FAIL("%s does not take %s (doublet operator id %d)", who, r->name, op);
  return r->clover != TMHIP_SW_NONE ? tmhip_ndsw_ready(ctx, who, true) : 0;
}
