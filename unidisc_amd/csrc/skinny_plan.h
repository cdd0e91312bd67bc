// How udm_gemm_skinny_bf16 (decode.hip) splits K over workgroups, as a pure function of the shape and of the workspace it is given.  Plain C++17, host
// only; tests/test_skinny_plan.py compiles this header alone (tests/skinny_plan_print.cpp) and holds kernels.skinny_ws_elems to it.
//   nblk    column tiles of 32 (grid.x)
//   S       K slices (grid.y): about two workgroups per CU (512 / nblk, rounded), each slice at least 128 deep, at most 32, at most the slabs the workspace
//           holds, cap = ws_elems / (M N); 1 without a workspace or with 512 column tiles and more
//   kslice  K per slice, a multiple of 32; S is then re-derived as ceil(K / kslice) so that no slice is empty
// M enters through cap alone: with a workspace of skinny_plan_ws_elems(M, N, K) elements, or more, the plan of (M, N, K) is the plan of every M' <= M on
// the same (N, K) - the row halves [0, 64) and [64, M) of a 65..128-row call are split as two calls on those rows would be.
#pragma once

struct SkinnyPlan {
  long nblk = 1;
  long S = 1;
  long kslice = 32;
};

// the slices wanted before the workspace bounds them (1: never split)
inline long skinny_plan_s_wanted(long N, long K) {
  const long nblk = (N + 31) / 32;
  if (nblk >= 512) return 1;
  long S = (512 + nblk / 2) / nblk;
  S = S < K / 128 ? S : K / 128;
  S = S < 32 ? S : 32;
  return S < 1 ? 1 : S;
}

inline SkinnyPlan skinny_plan(long M, long N, long K, bool have_ws, long ws_elems) {
  SkinnyPlan pl;
  pl.nblk = (N + 31) / 32;
  long S = 1;
  if (have_ws && pl.nblk < 512) {
    S = skinny_plan_s_wanted(N, K);
    const long cap = ws_elems / (M * N);
    if (S > cap) S = cap;
    if (S < 1) S = 1;
  }
  pl.kslice = ((K + S - 1) / S + 31) / 32 * 32;
  pl.S = (K + pl.kslice - 1) / pl.kslice;
  return pl;
}

// fp32 elements that leave the plan unbounded by the workspace (0: it does not split)
inline long skinny_plan_ws_elems(long M, long N, long K) {
  const long S = skinny_plan_s_wanted(N, K);
  return S > 1 ? S * M * N : 0;
}
