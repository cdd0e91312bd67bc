// Prints the launch plan of udm_reveal_rows (unidisc_amd/csrc/reveal_plan.h) for the row lengths on stdin, one per line:
//   L -> L= threads= vpt= lds= ok=          (tests/test_reveal_plan.py; plain C++17, no HIP)
#include "reveal_plan.h"

#include <stdio.h>

int main() {
  long L;
  while (scanf("%ld", &L) == 1) {
    const RevealPlan p = reveal_plan(L);
    printf("L=%ld threads=%d vpt=%d lds=%u ok=%d\n", L, p.threads, p.vpt, p.lds_bytes, (int)p.ok);
  }
  return 0;
}
