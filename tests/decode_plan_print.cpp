// Prints the key split of the decode attention (unidisc_amd/csrc/decode_plan.h) for the cases on stdin, one per line:
//   n BH cap -> n= BH= cap= S= chunk= bound=      bound = decode_plan_s_bound(BH, n, cap), n read as Lmax
//   (tests/test_decode_plan.py; plain C++17, no HIP)
#include "decode_plan.h"

#include <stdio.h>

int main() {
  long n, BH, cap;
  while (scanf("%ld %ld %ld", &n, &BH, &cap) == 3) {
    const DecodePlan p = decode_plan(n, BH, cap);
    printf("n=%ld BH=%ld cap=%ld S=%ld chunk=%ld bound=%ld\n", n, BH, cap, p.S, p.chunk, decode_plan_s_bound(BH, n, cap));
  }
  return 0;
}
