// Prints the K split of the skinny GEMM (unidisc_amd/csrc/skinny_plan.h) for the cases on stdin, one per line:
//   M N K ws_elems -> M= N= K= ws= nblk= S= kslice= need=      ws_elems < 0: no workspace; need = skinny_plan_ws_elems(M, N, K)
//   (tests/test_skinny_plan.py; plain C++17, no HIP)
#include "skinny_plan.h"

#include <stdio.h>

int main() {
  long M, N, K, ws;
  while (scanf("%ld %ld %ld %ld", &M, &N, &K, &ws) == 4) {
    const SkinnyPlan p = skinny_plan(M, N, K, ws >= 0, ws < 0 ? 0 : ws);
    printf("M=%ld N=%ld K=%ld ws=%ld nblk=%ld S=%ld kslice=%ld need=%ld\n", M, N, K, ws, p.nblk, p.S, p.kslice, skinny_plan_ws_elems(M, N, K));
  }
  return 0;
}
