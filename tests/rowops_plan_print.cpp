// Prints the row-kernel launch plan (unidisc_amd/csrc/rowops_plan.h) of the calls on stdin, one per line:  entry M d L a b ws_elems name
//   entry (a, b):  fwd (-, -) | norm_bwd (modulated, -) | residual_bwd (gated, sandwich) | norm_residual_bwd (-, -) | norm_residual_bwd_ada (-, -) |
//                  qk_fwd (qk_norm, -) | qk_bwd (qk_norm, contiguous gradients)
// -> name form= inst= grid= bpb= ws= lds= reduce= need= ok=          (tests/test_rowops_plan.py; plain C++17, no HIP)
#include "rowops_plan.h"

#include <stdio.h>
#include <string.h>

int main() {
  char entry[64], name[256];
  long M, d, L, ws;
  int a, b;
  while (scanf("%63s %ld %ld %ld %d %d %ld %255s", entry, &M, &d, &L, &a, &b, &ws, name) == 8) {
    RowPlan p;
    if (!strcmp(entry, "fwd")) p = row_plan_fwd(M, d);
    else if (!strcmp(entry, "norm_bwd")) p = row_plan_norm_bwd(M, d, L, a, ws);
    else if (!strcmp(entry, "residual_bwd")) p = row_plan_residual_bwd(M, d, L, a, b, ws);
    else if (!strcmp(entry, "norm_residual_bwd")) p = row_plan_norm_residual_bwd(M, d);
    else if (!strcmp(entry, "norm_residual_bwd_ada")) p = row_plan_norm_residual_bwd_ada(M, d, L);
    else if (!strcmp(entry, "qk_fwd")) p = row_plan_qk_fwd(M, d, a);
    else if (!strcmp(entry, "qk_bwd")) p = row_plan_qk_bwd(M, d, a, b, ws);
    else { fprintf(stderr, "unknown entry point %s\n", entry); return 1; }
    const char* form = p.form == WAVE_ROW ? "WAVE_ROW" : (p.form == BLOCK_ROW ? "BLOCK_ROW" : "BLOCK_ROW_2ROWS");
    printf("%s form=%s inst=%d grid=%u bpb=%d ws=%d lds=%u reduce=%ux%u need=%ld ok=%d\n", name, form, p.inst, p.grid, p.bpb, (int)p.use_ws, p.lds_bytes,
           p.reduce_rows, p.reduce_cols, p.ws_need, (int)p.ok);
  }
  return 0;
}
