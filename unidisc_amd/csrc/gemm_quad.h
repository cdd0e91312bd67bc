// Internal interface between gemm.hip (dispatch, C ABI) and gemm_quad.hip (one-wave-per-SIMD kernels).  Not part of the C ABI.
#pragma once
#include "common.h"
#include "gemm_plan.h"

struct QuadArgs {
  const bf16_t* A;
  const bf16_t* B;
  void* C;
  const float* bias;   // EPI_BIAS / EPI_BIAS_GELU: fp32 [N] input; EPI_DGELU: fp32 [N] OUTPUT receiving the column sums (or null)
  bf16_t* aux;
  long lda, ldb, ldc, ldaux;
  int M, N, K;
  int tiles_m, tiles_n;
  float beta;
  int splitk;          // > 1 (fp32 output only): K cut into slices, slice s stores its partial tile at C + s * slice_stride
  long slice_stride;
  int group_m;
  // paired launch (TN wgrad form): a SECOND problem with the same N and K stacked below the first one's row tiles - tiles [0, tiles_m_split) of the tile rows are
  // problem one, the rest problem two (its own operands and output).  One launch of exactly 256 tiles instead of a 256-tile launch of 192-row tiles plus a
  // split-K launch + reduce (qkv and out-proj weight gradients: 192 + 64 tiles of 256 x 256).  0 = single problem.
  int tiles_m_split = 0;
  // multi-problem launch (TN wgrad form, 256 x 256 tiles): up to four problems C_i[M_i, N_i] = A_i[K, M_i]^T B_i[K, N_i] over the SAME K share one grid (and one
  // K split) - the four few-tile weight gradients of a small DiT block (UniDisc-S: 27 + 9 + 36 + 36 tiles over K = 24 576).  Tiles of problem i are
  // [m_tile_start[i], m_tile_start[i + 1]); 0 = off.
  int nprob = 0;
  int m_tile_start[5] = {0, 0, 0, 0, 0};
  int m_tiles_n[4] = {0, 0, 0, 0};
  const bf16_t* mA[4] = {nullptr, nullptr, nullptr, nullptr};
  const bf16_t* mB[4] = {nullptr, nullptr, nullptr, nullptr};
  void* mC[4] = {nullptr, nullptr, nullptr, nullptr};
  long mlda[4] = {0, 0, 0, 0}, mldb[4] = {0, 0, 0, 0}, mldc[4] = {0, 0, 0, 0};
  const bf16_t* A2 = nullptr;
  const bf16_t* B2 = nullptr;
  void* C2 = nullptr;
  long lda2 = 0, ldb2 = 0, ldc2 = 0;
  unsigned* timeline = nullptr;   // diagnostic build of the asm K loop (make UDM_QUADLOOP=timeline)
};

extern unsigned* g_quad_timeline;
int udm_gemm_cus_available();   // GemmEnv::cus of gemm.hip: 256, or the cap of udm_gemm_set_cus / UDM_GEMM_CUS (attention.hip plans against it too)
// launch the one-wave-per-SIMD kernel a plan of gemm_plan.h names (GEMM_QUAD / GEMM_QUAD_RAGGED: fm, grid, LDS, slices, asm K loop) in the given operand form.
// NT takes every epilogue (fp32 output: none); TN is fp32 without an epilogue; NN is plain, bf16 or (out_f32: the partial tiles of a K split) fp32.
enum { QUAD_NT = 0, QUAD_TN = 1, QUAD_NN = 2 };
int udm_quad_launch(const QuadArgs& a, const GemmPlan& p, int form, int epilogue, int out_f32, hipStream_t stream);
