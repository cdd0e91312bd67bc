// Prints attn_kv_causal_walk_end (unidisc_amd/csrc/attention_plan.h) for every 1 <= Lq <= Lk <= max_l (argv[1]), then for the (Lq, Lk) pairs that follow
// on the command line, and every 128-query tile, one line each:
//   Lq Lk q_tile end                                      (tests/test_attention_kv_causal_plan.py; plain C++17, no HIP)
#include "attention_plan.h"

#include <stdio.h>
#include <stdlib.h>

static_assert(attn_kv_causal_walk_end(129, 193, 0) == 3 && attn_kv_causal_walk_end(129, 193, 1) == 4, "usable in constant expressions, as the kernel uses it");

int main(int argc, char** argv) {
  const long max_l = argc > 1 ? atol(argv[1]) : 320;
  for (long Lk = 1; Lk <= max_l; ++Lk)
    for (long Lq = 1; Lq <= Lk; ++Lq)
      for (long t = 0; t < (Lq + 127) / 128; ++t) printf("%ld %ld %ld %ld\n", Lq, Lk, t, attn_kv_causal_walk_end(Lq, Lk, t));
  for (int a = 2; a + 1 < argc; a += 2) {   // further (Lq, Lk) pairs, past max_l
    const long Lq = atol(argv[a]), Lk = atol(argv[a + 1]);
    for (long t = 0; t < (Lq + 127) / 128; ++t) printf("%ld %ld %ld %ld\n", Lq, Lk, t, attn_kv_causal_walk_end(Lq, Lk, t));
  }
  return 0;
}
