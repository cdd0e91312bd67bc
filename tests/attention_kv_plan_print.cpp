// Prints attn_plan_fwd_kv (unidisc_amd/csrc/attention_plan.h) for the problems on stdin, one per line:  D B H Lq Lk name
// -> name D= q_tiles= kv_tiles= grid= lds= wgs= grid_ok=          (tests/test_attention_kv_plan.py; plain C++17, no HIP)
#include "attention_plan.h"

#include <stdio.h>

int main() {
  int D;
  long B, H, Lq, Lk;
  char name[256];
  while (scanf("%d %ld %ld %ld %ld %255s", &D, &B, &H, &Lq, &Lk, name) == 6) {
    const AttnKvPlan p = attn_plan_fwd_kv(AttnKvProblem{D, B, H, Lq, Lk});
    printf("%s D=%d q_tiles=%u kv_tiles=%u grid=%u lds=%u wgs=%d grid_ok=%d\n", name, p.D, p.q_tiles, p.kv_tiles, p.grid, p.lds_bytes,
           ATTN_KV_WGS(p.D), (int)p.grid_ok);
  }
  return 0;
}
