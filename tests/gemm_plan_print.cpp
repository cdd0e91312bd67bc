// Prints the GEMM launch plan (unidisc_amd/csrc/gemm_plan.h) of the calls on stdin, one per line:
//   entry name  cus quad persist tile ragged asm  n  arg_1 .. arg_n
//   nt         M N K ldc ldaux epilogue out_f32 beta        tn         M N K beta
//   nt_splitk  M N K ldc ws_elems                           tn_splitk  M N K ldc ws_elems
//   nn         M N K                                        nn_splitk  M N K ldc ws_elems
//   tn_pair    M0 M1 N K contiguous ws_elems                tn_multi   K ws_elems M_1 N_1 .. M_p N_p
//   slices     tiles K depth cus   (the slice rule alone: printed as splitk=)
// -> name family= rows= asm= tiles= grid= lds= splitk= finish= reduce= rgrid= need= fallback= ok=      (tests/test_gemm_plan.py; plain C++17, no HIP)
#include "gemm_plan.h"

#include <stdio.h>
#include <string.h>

int main() {
  char entry[64], name[256];
  GemmEnv env;
  int n;
  while (scanf("%63s %255s %d %d %d %d %d %d %d", entry, name, &env.cus, &env.quad, &env.persist, &env.force_tile, &env.ragged, &env.quad_asm, &n) == 9) {
    long a[16] = {0};
    if (n < 0 || n > 16) { fprintf(stderr, "%s: too many arguments\n", name); return 1; }
    for (int i = 0; i < n; ++i)
      if (scanf("%ld", &a[i]) != 1) { fprintf(stderr, "%s: short line\n", name); return 1; }
    GemmPlan p;
    if (!strcmp(entry, "nt")) p = gemm_plan_nt(a[0], a[1], a[2], a[3], a[4], (int)a[5], a[6] != 0, a[7] != 0, env);
    else if (!strcmp(entry, "tn")) p = gemm_plan_tn(a[0], a[1], a[2], (float)a[3], env);
    else if (!strcmp(entry, "nt_splitk")) p = gemm_plan_nt_splitk(a[0], a[1], a[2], a[3], a[4], env);
    else if (!strcmp(entry, "tn_splitk")) p = gemm_plan_tn_splitk(a[0], a[1], a[2], a[3], a[4], env);
    else if (!strcmp(entry, "nn")) p = gemm_plan_nn(a[0], a[1], a[2], env);
    else if (!strcmp(entry, "nn_splitk")) p = gemm_plan_nn_splitk(a[0], a[1], a[2], a[3], a[4], env);
    else if (!strcmp(entry, "tn_pair")) p = gemm_plan_tn_pair(a[0], a[1], a[2], a[3], a[4] != 0, a[5], env);
    else if (!strcmp(entry, "tn_multi")) {
      int64_t M[4], N[4];
      const int np = (n - 2) / 2;
      if (np < 1 || np > 4) { fprintf(stderr, "%s: one to four problems\n", name); return 1; }
      for (int i = 0; i < np; ++i) { M[i] = a[2 + 2 * i]; N[i] = a[3 + 2 * i]; }
      p = gemm_plan_tn_multi(np, M, N, a[0], a[1], env);
    } else if (!strcmp(entry, "slices")) p.splitk = gemm_splitk_slices(a[0], a[1], (int)a[2], (int)a[3]);
    else { fprintf(stderr, "unknown entry point %s\n", entry); return 1; }
    static const char* const family[] = {"SMALL", "STAGGER", "PERSIST", "QUAD", "QUAD_RAGGED"};
    static const char* const finish[] = {"none", "atomics", "ws"};
    static const char* const reduce[] = {"none", "f32", "bf16", "multi"};
    printf("%s family=%s rows=%d asm=%d tiles=%dx%d grid=%u lds=%u splitk=%d finish=%s reduce=%s rgrid=%u+%u need=%ld fallback=%d ok=%d\n", name, family[p.family], p.tile_rows,
           p.asm_loop, p.tiles_m, p.tiles_n, p.grid, p.lds_bytes, p.splitk, finish[p.finish], reduce[p.reduce], p.reduce_grid, p.reduce_grid2, p.ws_need, (int)p.fallback, (int)p.ok);
  }
  return 0;
}
