// Prints the key-split plan (unidisc_amd/csrc/attention_plan.h) for the problems on stdin, one per line:  D B H Lq Lk cus splits ws_elems name
//   splits = 0: attn_plan_fwd_kv_split(problem, cus); splits >= 1: that count through attn_kv_split_clamp with a workspace of ws_elems floats (-1: unlimited,
//   -2: the NULL workspace)
// -> name S= auto= grid= unsplit_grid= kv_tiles= ws= grid_ok= ranges=b0-e0,b1-e1,...          (tests/test_attention_kv_split_plan.py; plain C++17, no HIP)
#include "attention_plan.h"

#include <limits.h>
#include <stdio.h>

int main() {
  int D, cus;
  long B, H, Lq, Lk, splits, ws;
  char name[256];
  while (scanf("%d %ld %ld %ld %ld %d %ld %ld %255s", &D, &B, &H, &Lq, &Lk, &cus, &splits, &ws, name) == 9) {
    const AttnKvProblem prob{D, B, H, Lq, Lk};
    const AttnKvSplitPlan chosen = attn_plan_fwd_kv_split(prob, cus);
    const long want = splits > 0 ? splits : (long)chosen.splits;
    const long S = attn_kv_split_clamp(prob, want, ws != -2, ws < 0 ? LONG_MAX : ws);
    const AttnKvSplitPlan p = attn_kv_split_with(prob, S);
    printf("%s S=%u auto=%u grid=%u unsplit_grid=%u kv_tiles=%u ws=%ld grid_ok=%d ranges=", name, p.splits, chosen.splits, p.grid, p.base.grid, p.base.kv_tiles, p.ws_elems,
           (int)p.grid_ok);
    for (long s = 0; s < S; ++s) {
      long b, e;
      attn_kv_split_range(p.base.kv_tiles, S, s, b, e);
      printf("%s%ld-%ld", s ? "," : "", b, e);
    }
    printf("\n");
  }
  return 0;
}
