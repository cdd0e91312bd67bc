// Which kernel one GEMM entry point of gemm.hip (udm_gemm_nt_bf16 ... udm_gemm_tn_multi_bf16) launches and with what numbers, as a pure host function of the shape,
// the leading dimensions, the epilogue, the output type, beta, the workspace offered and the process-wide switches (GemmEnv).  Plain C++17 without HIP, globals or
// getenv: gemm.hip / gemm_quad.hip execute the plan, tests/test_gemm_plan.py compiles this header alone and prints the plan of every shape the GPU tests use.
// unidisc_amd/kernels.py (GEMM_WS, _splitk_slices) sizes the workspace it offers after the slice rule below; the same test holds the two together.
//   GEMM_SMALL        gemm_nt_kernel: 128 x 128 tiles, register-staged, 4 waves; any K % 8 == 0
//   GEMM_STAGGER      gemm_nt_stagger_kernel: (192 | 256 | 320) x 256 tiles, 8 waves, LDS-DMA, one block per tile (x slice); NT and TN
//   GEMM_PERSIST      the same kernel's persistent wide form: `cus` blocks walk whole tiles, 16-byte epilogue accesses; NT only
//   GEMM_QUAD         gemm_quad_kernel: one wave per SIMD, (192 | 256 | 320) x 256 whole tiles (fm = rows / 64); NT, TN and NN
//   GEMM_QUAD_RAGGED  its 320-row form with a ragged last tile row (written fm = -5 at the call sites); NT and NN, plain / bias epilogue, bf16 output
#pragma once
#include <stdint.h>

// everything process-wide a decision depends on; gemm.hip fills it in one place (gemm_env_from_environment) and the setters write into it
struct GemmEnv {
  int cus = 256;         // CUs the GEMMs may plan for: 256, or the cap of udm_gemm_set_cus / UDM_GEMM_CUS (a multiple of 8 in [8, 256])
  int quad = 1;          // one-wave-per-SIMD kernels: 0 off, 1 where they fill the chip, 2 wherever the shape fits (udm_gemm_set_quad / UDM_GEMM_QUAD)
  int persist = 1;       // 0: one block per output tile everywhere (udm_gemm_set_persist / UDM_GEMM_PERSIST)
  int force_tile = -1;   // udm_gemm_set_tile: -1 auto, 0 the 128 x 128 kernel, 192 / 256 / 320
  int ragged = 1;        // 0: whole quad tiles only (UDM_QUAD_RAGGED)
  int quad_asm = 1;      // generated asm K loop: 0 the C++ loop everywhere, 1 the 32x32x16 statement, 2 the 16x16x32 statement where the build has it (UDM_QUAD_ASM)
  int group_m = 0;       // tile-row grouping of the block order, 0 = the kernels' default (UDM_GEMM_GROUP_M)
};

enum GemmFamily { GEMM_SMALL, GEMM_STAGGER, GEMM_PERSIST, GEMM_QUAD, GEMM_QUAD_RAGGED };
enum GemmFinish { GEMM_FINISH_NONE, GEMM_FINISH_ATOMICS, GEMM_FINISH_WS };               // how partial sums of a K split reach C: fp32 atomics into C / workspace + reduce
enum GemmReduce { GEMM_REDUCE_NONE, GEMM_REDUCE_F32, GEMM_REDUCE_BF16, GEMM_REDUCE_MULTI };   // splitk_reduce_kernel / _bf16_kernel / _multi_kernel
enum { GEMM_EPI_NONE = 0, GEMM_EPI_BIAS = 1, GEMM_EPI_BIAS_GELU = 2, GEMM_EPI_DGELU = 3 };     // = UDM_EPI_* of include/unidisc_hip.h

struct GemmPlan {
  GemmFamily family = GEMM_SMALL;
  int tile_rows = 0;          // 128 / 192 / 256 / 320; the quad kernels' fm = tile_rows / 64
  int asm_loop = 0;           // GEMM_QUAD: 0 the C++ K loop, 1 / 2 the generated statement
  int tiles_m = 0, tiles_n = 0;
  uint32_t grid = 0;          // blocks: tiles x slices, or `cus` persistent blocks
  uint32_t lds_bytes = 0;
  int splitk = 1;
  GemmFinish finish = GEMM_FINISH_NONE;
  GemmReduce reduce = GEMM_REDUCE_NONE;
  uint32_t reduce_grid = 0, reduce_grid2 = 0;   // (the pair reduces its two outputs in two launches)
  long ws_need = 0;           // floats of the workspace the launch writes and the reduction reads
  int group_m = 0;
  bool fallback = false;      // the split entry point hands the call to the plain entry point (udm_gemm_nt_bf16 / _tn_ / _nn_), whose plan applies
  bool ok = false;            // a launch exists (pair / multi: false = return 3, nothing launched; nn: udm_gemm_nn_ok)
  int fm() const { return family == GEMM_QUAD_RAGGED ? -(tile_rows / 64) : tile_rows / 64; }
};

constexpr int GEMM_BK = 64;                 // K tile of every kernel; the LDS-DMA kernels have no K tail and need two K tiles (K % 64 == 0, K >= 128)
constexpr int GEMM_CUS = 256;
constexpr int GEMM_SMALL_SLOTS = 512;       // co-resident 128 x 128 blocks on the chip (2 per CU)
constexpr int GEMM_SMALL_LDS = 4 * 128 * GEMM_BK * 2;
constexpr int GEMM_BIG_MIN = 192;           // M, N below it take the 128 x 128 kernel
constexpr int GEMM_QUAD_MIN_TILES = 128;    // auto mode: the quad kernels only where their tiles fill at least half the chip ...
constexpr int GEMM_QUAD_MAX_TILES = 256;    // ... and (NT) at most one round: multi-round shapes stay with the persistent 8-wave blocks
constexpr double GEMM_RAGGED_PENALTY = 1.03;   // a ragged 320-row round against a whole-tile round of the same height
constexpr int GEMM_SLICES_MAX = 32;
constexpr int GEMM_SLICE_DEPTH = 8;         // K tiles per slice at least: NT, TN, pair, multi
constexpr int GEMM_SLICE_DEPTH_NN = 4;      // udm_gemm_nn_splitk_bf16 (the leftover tile rows of a row-split dgrad: K = 2048 is 32 K tiles, 4 tiles -> 8 slices)
constexpr int GEMM_REDUCE_GRID_MAX = 2048;
constexpr int GEMM_MULTI_MAX_TILES = 128;   // udm_gemm_tn_multi_bf16: more tiles than half the chip are no few-tile problem
// udm_gemm_tn_bf16, beta = 1: fp32 atomics into C.  Measured on MI355X (2048 x 2048 output, K = 10240): a 4-way split + fp32 atomics is SLOWER (0.31 ms) than one
// slice per tile on a quarter of the CUs (0.24 ms) - 16.8 M L2 atomics cost more than the idle CUs.  Only split when the output is tiny.
constexpr int GEMM_ATOMIC_BLOCKS_MAX = 32, GEMM_ATOMIC_SLICE_DEPTH = 16, GEMM_ATOMIC_SLICES_MAX = 8;

inline long gemm_cdiv(long a, long b) { return (a + b - 1) / b; }
inline uint32_t gemm_lds_big(int tile_rows) { return (uint32_t)(2 * (tile_rows + 256) * GEMM_BK * 2); }   // two stages of an A and a B tile (stagger and quad alike)
inline uint32_t gemm_reduce_grid(long elems) { const long g = gemm_cdiv(elems / 4, 256); return (uint32_t)(g < GEMM_REDUCE_GRID_MAX ? g : GEMM_REDUCE_GRID_MAX); }
inline bool gemm_dma_k_ok(long K) { return K % GEMM_BK == 0 && K >= 2 * GEMM_BK; }

// THE rounds cost: `tiles` tiles of `tile_rows` rows on `slots` co-resident blocks take ceil(tiles / slots) rounds, a round as long as the tile is high
inline long gemm_round_cost(long tiles, long slots, long tile_rows) { return gemm_cdiv(tiles, slots) * tile_rows; }

// THE split-K slice rule: as many slices as fill `cus` CUs once (any count: slices may be uneven), each at least `depth` K tiles deep, at most 32; below 2: no split.
// The call sites differ in two arguments: depth 4 for NN and 8 elsewhere; the pair counts against 256 CUs whatever the cap.
inline int gemm_splitk_slices(long tiles, long K, int depth, int cus) {
  long s = tiles > 0 ? cus / tiles : 1;
  if (s > K / GEMM_BK / depth) s = K / GEMM_BK / depth;
  if (s > GEMM_SLICES_MAX) s = GEMM_SLICES_MAX;
  return s < 2 ? 1 : (int)s;
}

// more than one round of whole 256- / 320-row tiles: the shape the persistent form exists for (what the cost model credits) ...
inline bool gemm_persistent_shape(int tile_rows, long M, long N) {
  return tile_rows >= 256 && M % tile_rows == 0 && N % 256 == 0 && (M / tile_rows) * (N / 256) > GEMM_CUS;
}
// ... and THE predicate of the launch: that shape, switched on, unsplit, with leading dimensions its 16-byte epilogue accesses accept.  The cost model credits the
// shape alone: a forced one-block-per-tile run (persist = 0) or a narrow ldc keeps the tile the persistent form would have had.
inline bool gemm_persistent_wide_ok(int tile_rows, long M, long N, long K, long ldc, long ldaux, int epi, bool out_f32, int splitk, const GemmEnv& env, bool wide_epilogue = true) {
  const bool aux_ok = epi < GEMM_EPI_BIAS_GELU || ldaux % 8 == 0;
  return env.persist && splitk <= 1 && gemm_persistent_shape(tile_rows, M, N) && K / GEMM_BK >= 2 && (!wide_epilogue || ((out_f32 ? ldc % 4 == 0 : ldc % 8 == 0) && aux_ok));
}

// THE tile cost model of the 8-wave kernels: the tile whose tile count wastes the least of the 256-CU rounds; 0 = the 128 x 128 kernel
inline int gemm_choose_tile(long M, long N, long K, const GemmEnv& env) {
  if (!gemm_dma_k_ok(K)) return 0;   // the LDS-DMA path has no K-tail handling: such shapes take the register-staged kernel
  if (env.force_tile >= 0) return env.force_tile;
  if (M < GEMM_BIG_MIN || N < GEMM_BIG_MIN) return 0;
  const double eff[4] = {0.74, 0.93, 1.0, 1.0};  // measured relative throughput of {128x128, 192, 256, 320} x 256 tiles at full occupancy
  const int bms[4] = {128, 192, 256, 320};
  double best = 1e30;
  int pick = 0;
  for (int c = 0; c < 4; ++c) {
    const long tiles = gemm_cdiv(M, bms[c]) * gemm_cdiv(N, c == 0 ? 128 : 256);
    double t = gemm_round_cost(tiles, c == 0 ? GEMM_SMALL_SLOTS : GEMM_CUS, bms[c]) * (c == 0 ? 128 : 256) * (c == 0 ? 2.0 : 1.0) / eff[c];  // time ~ rounds x tile area (2 blocks/CU share a CU)
    // short contractions (UniDisc-S: K = 768, 12 K tiles per output tile): prologue and epilogue are a large part of a tile, and only the persistent
    // form (256- / 320-row tiles, whole tiles, more than one round) overlaps the next tile's first loads with them.  Measured at M = 24576
    // (scripts/bench_gemm_s.py): N = 3072 + GELU 162 us persistent 256 vs 178 (192) / 194 (320, ragged); + GELU' 166 vs 187 / 228; N = 2304 plain 111 vs 120 / 114.
    const bool persistent = gemm_persistent_shape(bms[c], M, N);
    if (K <= 1024 && !persistent) t *= 1.15;
    // ... and at any K the persistent form (next tile's first loads under the epilogue, wide epilogue) is worth ~10 % of a launch: M = 9216 (config E), K = 2048,
    // N = 8192 + GELU: 293 us as 5 rounds of persistent 256-row tiles against 313 us as 6 rounds of 192-row tiles (GELU' + column sums 290 vs 316); N = 6144 plain:
    // 207 us (4 rounds of 256) against 217 (3 rounds of ragged 320) - scripts/bench_gemm_epi.py with M / N / TILE from the environment
    if (persistent) t *= 0.90;
    if (t < best || (t == best && c > 0)) { best = t; pick = c == 0 ? 0 : bms[c]; }  // ties go to the larger tile (fewer operand re-reads)
  }
  return pick;
}

// whole quad tiles: the height / 64 (fm_max .. 3) that fills whole rounds of the available CUs best (ties: the larger wave tile); 0 = none fits.
// fm_max = 5 for NT and NN, 4 for TN (FM = 5 spills in the TN form: 2 x 9 fragment halves beside 320 accumulators)
inline int gemm_quad_whole_fm(long M, long N, long K, int fm_max, const GemmEnv& env) {
  if (!env.quad || !gemm_dma_k_ok(K) || N % 256 != 0) return 0;
  long best = 0;
  int pick = 0;
  for (int fm = fm_max; fm >= 3; --fm) {
    const int bm = 64 * fm;
    if (M % bm != 0) continue;
    const long t = gemm_round_cost((M / bm) * (N / 256), env.cus, bm);
    if (!pick || t < best) { best = t; pick = fm; }
  }
  return pick;
}
// NN (and the ragged NT gate): 3 / 4 / 5 whole tiles, or -5: 320-row tiles with a ragged last tile row, where that is fewer rounds x rows than any whole-tile height
inline int gemm_quad_nn_fm(long M, long N, long K, const GemmEnv& env) {
  const int whole = gemm_quad_whole_fm(M, N, K, 5, env);
  if (env.ragged && env.quad && gemm_dma_k_ok(K) && N % 256 == 0 && M > 320 && M % 320 != 0) {
    const long tiles = gemm_cdiv(M, 320) * (N / 256);
    const double best = whole ? (double)gemm_round_cost((M / (64 * whole)) * (N / 256), env.cus, 64 * whole) : 1e30;
    if (tiles >= GEMM_QUAD_MIN_TILES && (double)gemm_round_cost(tiles, env.cus, 320) * GEMM_RAGGED_PENALTY < best) return -5;
  }
  return whole;
}

inline GemmPlan gemm_plan_launch(GemmFamily family, int tile_rows, long tiles_m, long tiles_n, int splitk, const GemmEnv& env) {
  GemmPlan p;
  p.family = family; p.tile_rows = tile_rows; p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n; p.splitk = splitk; p.group_m = env.group_m; p.ok = true;
  p.grid = family == GEMM_PERSIST ? (uint32_t)env.cus : (uint32_t)(tiles_m * tiles_n * (splitk > 1 ? splitk : 1));
  p.lds_bytes = family == GEMM_SMALL ? GEMM_SMALL_LDS : gemm_lds_big(tile_rows);
  return p;
}
// a quad launch of M x N outputs, fm = 3 / 4 / 5 or -5
inline GemmPlan gemm_plan_quad(int fm, long M, long N, int splitk, const GemmEnv& env) {
  const int rows = 64 * (fm < 0 ? -fm : fm);
  return gemm_plan_launch(fm < 0 ? GEMM_QUAD_RAGGED : GEMM_QUAD, rows, fm < 0 ? gemm_cdiv(M, rows) : M / rows, N / 256, splitk, env);
}
inline GemmPlan gemm_plan_big(int tile_rows, long M, long N, int splitk, const GemmEnv& env) {
  return gemm_plan_launch(GEMM_STAGGER, tile_rows, gemm_cdiv(M, tile_rows), gemm_cdiv(N, 256), splitk, env);
}
// partial tiles of `area` floats per slice through the workspace, then `reduce`
inline GemmPlan gemm_plan_ws(GemmPlan p, long area, GemmReduce reduce) {
  p.finish = GEMM_FINISH_WS; p.reduce = reduce; p.ws_need = (long)p.splitk * area; p.reduce_grid = gemm_reduce_grid(area);
  return p;
}
inline GemmPlan gemm_plan_fallback() { GemmPlan p; p.fallback = true; p.ok = true; return p; }

// udm_gemm_nt_bf16: C[M, N] = A[M, K] B[N, K]^T with an epilogue
inline GemmPlan gemm_plan_nt(long M, long N, long K, long ldc, long ldaux, int epi, bool out_f32, bool beta_nonzero, const GemmEnv& env, bool wide_epilogue = true) {
  const int t8 = gemm_choose_tile(M, N, K, env);
  if (env.force_tile < 0 && !beta_nonzero) {
    // whole tiles: the one-wave-per-SIMD kernel where its tile count fills rounds of the chip at least as well.  Measured (scripts/bench_gemm_quad.py, 1.4 B shapes,
    // random operands): it wins 1-3 % on single-round shapes with a plain or bias epilogue and loses 3 % where the GELU / GELU' epilogue runs (one wave per SIMD has
    // nothing to overlap its VALU with); multi-round shapes stay with the persistent 8-wave blocks.  (This gate counts rounds of 256 CUs; the fm pick those available.)
    if (const int fm = gemm_quad_whole_fm(M, N, K, 5, env)) {
      const long qt = (M / (64 * fm)) * (N / 256);
      const bool cheaper = t8 == 0 || gemm_round_cost(qt, GEMM_CUS, 64 * fm) <= gemm_round_cost(gemm_cdiv(M, t8) * gemm_cdiv(N, 256), GEMM_CUS, t8);
      const bool fits = ldc % 4 == 0 && (epi < GEMM_EPI_BIAS_GELU || ldaux % 4 == 0) && !(out_f32 && epi != GEMM_EPI_NONE);
      if (fits && (env.quad == 2 || (qt >= GEMM_QUAD_MIN_TILES && qt <= GEMM_QUAD_MAX_TILES && cheaper && epi <= GEMM_EPI_BIAS))) {
        GemmPlan p = gemm_plan_quad(fm, M, N, 1, env);
        const long nk = K / GEMM_BK;   // the generated K loop: FM 4 / 5, at least 4 K tiles, an even count
        if (fm >= 4 && nk >= 4 && nk % 2 == 0) p.asm_loop = env.quad_asm;
        return p;
      }
    }
    // one round of 320-row tiles with a ragged last tile row (config E: M = 9216, N = 2048): the one-wave-per-SIMD kernel's ragged form instead of the 8-wave one
    const long rt = gemm_cdiv(M, 320) * gemm_cdiv(N, 256);
    if (!out_f32 && epi <= GEMM_EPI_BIAS && M % 320 != 0 && N % 256 == 0 && rt >= GEMM_QUAD_MIN_TILES && rt <= GEMM_QUAD_MAX_TILES && ldc % 4 == 0 && t8 == 320 &&
        gemm_quad_nn_fm(M, N, K, env) == -5)
      return gemm_plan_quad(-5, M, N, 1, env);
  }
  if (t8 == 0) return gemm_plan_launch(GEMM_SMALL, 128, gemm_cdiv(M, 128), gemm_cdiv(N, 128), 1, env);
  GemmPlan p = gemm_plan_big(t8, M, N, 1, env);
  if (gemm_persistent_wide_ok(t8, M, N, K, ldc, ldaux, epi, out_f32, 1, env, wide_epilogue)) { p.family = GEMM_PERSIST; p.grid = (uint32_t)env.cus; }
  return p;
}

// udm_gemm_tn_bf16: C[M, N] (fp32) = beta C + A[K, M]^T B[K, N]
inline GemmPlan gemm_plan_tn(long M, long N, long K, float beta, const GemmEnv& env) {
  if (env.force_tile < 0) {   // whole tiles that fill the chip: the one-wave-per-SIMD kernel
    const int fm = gemm_quad_whole_fm(M, N, K, 4, env);
    if (fm && ((M / (64 * fm)) * (N / 256) >= GEMM_QUAD_MIN_TILES || env.quad == 2)) return gemm_plan_quad(fm, M, N, 1, env);
  }
  int tile = gemm_choose_tile(M, N, K, env);
  if (tile == 0) tile = M <= 192 ? 192 : 256;  // the K-major path has no small-tile kernel; the large one handles any M, N by clamping
  int sk = 1;
  if (beta == 1.0f) {  // accumulate form: few output tiles over a long K -> split K, atomically add
    const long tiles = gemm_cdiv(M, tile) * gemm_cdiv(N, 256), nkt = K / GEMM_BK;
    while (tiles * sk * 2 <= GEMM_ATOMIC_BLOCKS_MAX && nkt / (sk * 2) >= GEMM_ATOMIC_SLICE_DEPTH && sk < GEMM_ATOMIC_SLICES_MAX) sk *= 2;
  }
  GemmPlan p = gemm_plan_big(tile, M, N, sk, env);
  if (sk > 1) p.finish = GEMM_FINISH_ATOMICS;
  return p;
}

// udm_gemm_nt_splitk_bf16: 320 x 256 tiles of the 8-wave kernel, fp32 partial tiles, a reduce pass that rounds to bf16 (and honours ldc)
inline GemmPlan gemm_plan_nt_splitk(long M, long N, long K, long ldc, long ws_elems, const GemmEnv& env) {
  const int sk = gemm_splitk_slices(gemm_cdiv(M, 320) * gemm_cdiv(N, 256), K, GEMM_SLICE_DEPTH, env.cus);
  if (sk == 1 || K % GEMM_BK != 0 || ws_elems < (long)sk * M * N || N % 4 != 0 || ldc % 4 != 0 || M < 320 || N < 256) return gemm_plan_fallback();
  return gemm_plan_ws(gemm_plan_big(320, M, N, sk, env), M * N, GEMM_REDUCE_BF16);
}

// udm_gemm_tn_splitk_bf16: quad tiles where they are whole (256-row tiles wherever those are: fewer partial-tile bytes per flop; UniDisc-S 23.84 vs 23.97 ms with the
// round-count pick), else 256-row tiles of the 8-wave kernel; no atomics (a 4-way atomic split measured slower than leaving 3/4 of the CUs idle)
inline GemmPlan gemm_plan_tn_splitk(long M, long N, long K, long ldc, long ws_elems, const GemmEnv& env) {
  int fm = env.force_tile < 0 ? gemm_quad_whole_fm(M, N, K, 4, env) : 0;
  if (fm && M % 256 == 0) fm = 4;
  const long tiles = fm ? (M / (64 * fm)) * (N / 256) : gemm_cdiv(M, 256) * gemm_cdiv(N, 256);
  const int sk = gemm_splitk_slices(tiles, K, GEMM_SLICE_DEPTH, env.cus);
  if (sk == 1 || ws_elems < (long)sk * M * N || ldc != N || (M * N) % 4 != 0) return gemm_plan_fallback();
  return gemm_plan_ws(fm ? gemm_plan_quad(fm, M, N, sk, env) : gemm_plan_big(256, M, N, sk, env), M * N, GEMM_REDUCE_F32);
}

// udm_gemm_nn_bf16 (ok = udm_gemm_nn_ok): C[M, N] bf16 = A[M, K] B[K, N] on the quad kernels
inline GemmPlan gemm_plan_nn(long M, long N, long K, const GemmEnv& env) {
  const int fm = M > 0 ? gemm_quad_nn_fm(M, N, K, env) : 0;
  return fm ? gemm_plan_quad(fm, M, N, 1, env) : GemmPlan{};
}
// udm_gemm_nn_splitk_bf16: whole tiles only; slices at least FOUR K tiles deep
inline GemmPlan gemm_plan_nn_splitk(long M, long N, long K, long ldc, long ws_elems, const GemmEnv& env) {
  const int fm = M > 0 ? gemm_quad_nn_fm(M, N, K, env) : 0;
  if (!fm) return GemmPlan{};
  const int sk = fm > 0 ? gemm_splitk_slices((M / (64 * fm)) * (N / 256), K, GEMM_SLICE_DEPTH_NN, env.cus) : 1;
  if (sk == 1 || ws_elems < (long)sk * M * N || ldc % 4 != 0) return gemm_plan_fallback();
  return gemm_plan_ws(gemm_plan_quad(fm, M, N, sk, env), M * N, GEMM_REDUCE_BF16);
}

// udm_gemm_tn_pair_bf16: the 256 x 256 quad tiles of two wgrads with the same N and K in one grid.  The slices fill 256 CUs whatever the cap (kernels.py does not
// pair while CUs are held: gemm_tn_pair_ok).  `contiguous`: ldc0 == ldc1 == N and a 16-byte aligned workspace; without the split the launch is unsplit.
inline GemmPlan gemm_plan_tn_pair(long M0, long M1, long N, long K, bool contiguous, long ws_elems, const GemmEnv& env) {
  if (!env.quad || M0 <= 0 || M1 <= 0 || M0 % 256 || M1 % 256 || N <= 0 || N % 256 || !gemm_dma_k_ok(K)) return GemmPlan{};
  const long area = (M0 + M1) * N;
  const int sk = gemm_splitk_slices(area / (256 * 256), K, GEMM_SLICE_DEPTH, GEMM_CUS);
  if (sk == 1 || ws_elems < sk * area || !contiguous) return gemm_plan_quad(4, M0 + M1, N, 1, env);
  GemmPlan p = gemm_plan_ws(gemm_plan_quad(4, M0 + M1, N, sk, env), area, GEMM_REDUCE_F32);
  p.reduce_grid = gemm_reduce_grid(M0 * N); p.reduce_grid2 = gemm_reduce_grid(M1 * N);
  return p;
}

// udm_gemm_tn_multi_bf16: up to four wgrads over the same K; all their 256 x 256 quad tiles in one grid (tiles_m = their count, tiles_n = 1), always split
inline GemmPlan gemm_plan_tn_multi(int nprob, const int64_t* M, const int64_t* N, long K, long ws_elems, const GemmEnv& env) {
  if (!env.quad || !gemm_dma_k_ok(K)) return GemmPlan{};
  long tiles = 0, area = 0;
  for (int i = 0; i < nprob; ++i) {
    if (M[i] <= 0 || N[i] <= 0 || M[i] % 256 || N[i] % 256) return GemmPlan{};
    tiles += (M[i] / 256) * (N[i] / 256);
    area += M[i] * N[i];
  }
  const int sk = gemm_splitk_slices(tiles, K, GEMM_SLICE_DEPTH, env.cus);
  if (tiles > GEMM_MULTI_MAX_TILES || sk < 2 || ws_elems < sk * area) return GemmPlan{};
  return gemm_plan_ws(gemm_plan_quad(4, tiles * 256, 256, sk, env), area, GEMM_REDUCE_MULTI);
}
