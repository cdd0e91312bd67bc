// Which kernel one row-kernel entry point of rowops.hip (udm_norm_fwd ... udm_qknorm_rope_bwd) launches and with what numbers, as a pure host function of the shape,
// the flags and the workspace offered.  Plain C++17 without HIP: rowops.hip executes the plan, tests/test_rowops_plan.py compiles this header alone and prints the
// plan of every shape the GPU tests use.  unidisc_amd/kernels.py (ROWOPS_WS) sizes the workspace it offers after the constants below; the same test holds the two together.
//   WAVE_ROW         one 64-lane wave per row, 4 rows per block; inst = chunks of 512 columns per row (NCH; NIT of the qk kernels: 64 half-head groups)
//   BLOCK_ROW        one 256-thread block per row (d >= 2048); inst = chunks of 2048 columns (NCB / NIB)
//   BLOCK_ROW_2ROWS  qknorm_rope_fwd_brow_rows_kernel: a block per group of `inst` rows (d = 2048)
#pragma once
#include <stdint.h>

constexpr int ROWS_PER_BLOCK = 4;  // 256 threads = 4 waves = 4 rows in flight per block

enum RowForm { WAVE_ROW, BLOCK_ROW, BLOCK_ROW_2ROWS };
struct RowPlan {
  RowForm form = WAVE_ROW;
  int inst = 0;             // the template instance of the form's kernel
  uint32_t grid = 0;        // blocks of 256 threads
  int bpb = 0;              // modulated / gated calls: blocks per batch element (grid = B bpb)
  bool use_ws = false;      // column sums as one partial row per block in the workspace, then a reduction; false: atomics
  uint32_t lds_bytes = 0;
  uint32_t reduce_rows = 0, reduce_cols = 0;   // with use_ws: the reduction reads [reduce_rows][reduce_cols] partials (per column-sum plane)
  long ws_need = 0;         // floats of the workspace the launch reads and writes
  bool ok = false;          // a kernel exists for the shape
};

constexpr int ROW_GRID_MAX = 2048;            // blocks of any wave-per-row grid
constexpr int ROW_WS_MIN_GRID = 64;           // short chains (few blocks) stay on atomics
constexpr int NORM_BWD_GRID_NARROW = 1024, NORM_BWD_GRID_WIDE = 512;   // d < 2048 / wider (measured: 48.6 vs 51.6 us at d = 768 with 1024 blocks, 60.7 vs 57.9 us at d = 2048)
constexpr int NORM_BWD_GRID_ATOMICS = 512;    // the unmodulated call without a workspace
constexpr int RESID_BWD_GRID_GATED = 1024;
// d = 2048 still fits a wave per row (32 values per lane): no block-wide reductions; measured 41.8 us vs 52.9 us for the
// block-per-row form without dropout, equal with dropout (Philox regeneration dominates there)
constexpr int RESID_BWD_GRID_D2048 = 1024;
constexpr int RESID_BWD_GRID_BROW = 1536;     // wide rows: block-per-row form (8 elements per thread, high occupancy)
constexpr int ROW_BROW_GRID_ATOMICS = 256;    // no workspace: keep the same-address atomic chains short
constexpr int RESID_BWD_GRID = 512, RESID_BWD_GRID_WS = 1024;   // the latter: wide grid, column sums through the workspace
// 3 blocks per CU: every block leaves a [3][d] fp32 partial for colreduce3, and at 1536 blocks that workspace (38 MB written + read per call) cost more
// than the extra occupancy gave (in the step: 3.95 ms at 1536 blocks, 4.12 at 1024, 3.73 at 768, 3.77 at 512)
constexpr int FUSED_BWD_GRID_BROW = 768, FUSED_BWD_GRID_WROW = 1024;
constexpr int FUSED_ADA_GRID = 768;           // partial-sum rows of the adaLN form: grid = B * max(1, min(768 / B, L))
constexpr int QK_FWD_GRID_2ROWS = 1024;       // two rows per block iteration, 1024 blocks (in the step: 1.08-1.10 ms against 1.22-1.24 for one row per iteration; 3 rows 1.18, 4 rows 1.41)
constexpr int QK_FWD_GRID_BROW = 2048, QK_FWD_GRID_WROW = 1024;
constexpr int QK_BWD_GRID_BROW = 1024;        // (swept 256 .. 2048 in the step: 2.92 / 1.91 / 1.69 / 1.60 / 1.88 / 1.82 / 1.87 ms per step at 256 / 512 / 768 / 1024 / 1280 / 1536 / 2048)
// narrow rows (wave per row): with a workspace the column sums go through it and the grid can be wide enough to hide HBM latency (a same-address
// atomic per block and column limited it to 256 blocks: 117 us at d = 768, M = 24576); without one, the short atomic chains stay
constexpr int QK_BWD_GRID_WROW_WS = 1024, QK_BWD_GRID_WROW_ATOMICS = 256;

inline long row_min(long a, long b) { return a < b ? a : b; }
inline long row_blocks(long rows) { return (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }
inline int grid_rows(long M) {
  const long g = row_blocks(M);
  return (int)(g < ROW_GRID_MAX ? (g < 1 ? 1 : g) : ROW_GRID_MAX);
}
inline int nch_for(long d) { return (int)((d + 511) / 512); }
// template instance of the wave-per-row kernels: NCH chunks of 512 columns; 2048 < d <= 4096 runs the 8-chunk instance, a wider row has none (0: the plan is not ok)
inline int nch_dispatch(long d) { const int n = nch_for(d); return n <= 4 ? n : (d <= 4096 ? 8 : 0); }
// blocks per batch element of a modulated / gated call (M = B L): as many as `grid` allows, at most `per_elem`
inline int row_bpb(long grid, long B, long per_elem) { const long b = row_min(grid / B, per_elem); return (int)(b > 1 ? b : 1); }
// a plan of `grid` blocks of the form's instance `inst` (0: no kernel for the shape); row_plan_ws: its column sums through `planes` x [grid][cols] floats of workspace
inline RowPlan row_plan(RowForm form, int inst, long grid, int bpb = 0, long lds_bytes = 0) {
  RowPlan p;
  p.form = form; p.inst = inst; p.grid = (uint32_t)grid; p.bpb = bpb; p.lds_bytes = (uint32_t)lds_bytes; p.ok = inst != 0;
  return p;
}
inline RowPlan row_plan_ws(RowPlan p, long cols, int planes = 1) {
  p.use_ws = true; p.reduce_rows = p.grid; p.reduce_cols = (uint32_t)cols; p.ws_need = (long)p.grid * cols * planes;
  return p;
}

// udm_norm_fwd, udm_residual_fwd, udm_residual_norm_fwd, udm_residual_norm_fwd_ada
inline RowPlan row_plan_fwd(long M, long d) { return row_plan(WAVE_ROW, nch_dispatch(d), grid_rows(M)); }
// udm_norm_bwd; modulated: whole blocks per batch element, M = B L (the caller checks)
inline RowPlan row_plan_norm_bwd(long M, long d, long L, bool modulated, long ws_elems) {
  long grid = row_min(grid_rows(M), d < 2048 ? NORM_BWD_GRID_NARROW : NORM_BWD_GRID_WIDE);
  const int bpb = modulated ? row_bpb(grid, M / L, row_blocks(L)) : 0;
  if (modulated) grid = M / L * bpb;
  const bool ws = ws_elems >= grid * d && grid >= ROW_WS_MIN_GRID;
  if (!ws && !modulated) grid = row_min(grid, NORM_BWD_GRID_ATOMICS);
  const RowPlan p = row_plan(WAVE_ROW, nch_dispatch(d), grid, bpb);
  return ws ? row_plan_ws(p, d) : p;
}
// udm_residual_bwd; gated: M = B L (the caller checks).  Only the sandwich norm has a column sum (dw_b); the gate gradient's sums stay in registers.
inline RowPlan row_plan_residual_bwd(long M, long d, long L, bool gated, bool sandwich, long ws_elems) {
  if (gated) {   // adaLN-Zero: whole blocks per batch element
    const int bpb = row_bpb(RESID_BWD_GRID_GATED, M / L, row_blocks(L));
    const RowPlan p = row_plan(WAVE_ROW, nch_dispatch(d), M / L * bpb, bpb);
    return sandwich && ws_elems >= (long)p.grid * d && p.grid >= ROW_WS_MIN_GRID ? row_plan_ws(p, d) : p;
  }
  if (d == 2048 && (!sandwich || ws_elems >= RESID_BWD_GRID_D2048 * d)) {
    const RowPlan p = row_plan(WAVE_ROW, 4, RESID_BWD_GRID_D2048);
    return sandwich ? row_plan_ws(p, d) : p;
  }
  if (d >= 2048 && d <= 4096) {
    const long g = row_min(M, RESID_BWD_GRID_BROW);
    if (sandwich && ws_elems >= g * d) return row_plan_ws(row_plan(BLOCK_ROW, d <= 2048 ? 1 : 2, g), d);
    return row_plan(BLOCK_ROW, d <= 2048 ? 1 : 2, sandwich ? row_min(g, ROW_BROW_GRID_ATOMICS) : g);
  }
  const int inst = d < 2048 ? nch_for(d) : 0;
  if (sandwich && grid_rows(M) >= RESID_BWD_GRID_WS && ws_elems >= RESID_BWD_GRID_WS * d) return row_plan_ws(row_plan(WAVE_ROW, inst, RESID_BWD_GRID_WS), d);
  return row_plan(WAVE_ROW, inst, row_min(grid_rows(M), RESID_BWD_GRID));
}
// udm_norm_residual_bwd: always through the workspace, three column-sum planes (dw | dw_b | dbias) of [grid][d]
inline RowPlan row_plan_norm_residual_bwd(long M, long d) {
  if (M <= 0 || !(d == 2048 || d == 4096 || (d % 8 == 0 && d >= 64 && d < 2048))) return RowPlan{};
  if (d < 2048) return row_plan_ws(row_plan(WAVE_ROW, nch_for(d), row_min(grid_rows(M), FUSED_BWD_GRID_WROW)), d, 3);
  return row_plan_ws(row_plan(BLOCK_ROW, d == 2048 ? 1 : 2, row_min(M, FUSED_BWD_GRID_BROW)), d, 3);
}
// udm_norm_residual_bwd_ada: the block-per-row form over whole batch elements, a row per block iteration; three more planes of [grid][d] (shift | scale | gate
// partials) behind the first three
inline RowPlan row_plan_norm_residual_bwd_ada(long M, long d, long L) {
  if (M <= 0 || L <= 0 || M % L != 0 || !(d == 2048 || d == 4096)) return RowPlan{};
  const int bpb = row_bpb(FUSED_ADA_GRID, M / L, L);
  return row_plan_ws(row_plan(BLOCK_ROW, d == 2048 ? 1 : 2, M / L * bpb, bpb), d, 6);
}
// the qk kernels: iterations of 64 lanes over the 2 d / 16 half-head groups of a q | k row; no kernel beyond 8 (d % 16 == 0: that is d <= 4096)
inline int qk_nit(long d) { return (int)((2 * (d / 16) + 63) / 64); }
inline bool qk_shape_ok(long d) { return d > 0 && d % 16 == 0 && qk_nit(d) <= 8; }
// udm_qknorm_rope_fwd; LDS: the four affine vectors
inline RowPlan row_plan_qk_fwd(long M, long d, bool qk_norm) {
  if (!qk_shape_ok(d)) return RowPlan{};
  const long lds = qk_norm ? 4 * d * (long)sizeof(float) : 0;
  if (d == 2048) return row_plan(BLOCK_ROW_2ROWS, 2, row_min((M + 1) / 2, QK_FWD_GRID_2ROWS));
  if (d > 2048) return row_plan(BLOCK_ROW, 2, row_min(M, QK_FWD_GRID_BROW), 0, lds);
  return row_plan(WAVE_ROW, qk_nit(d), row_min(grid_rows(M), QK_FWD_GRID_WROW), 0, lds);
}
// udm_qknorm_rope_bwd; contiguous: dgq | dbq | dgk | dbk are one allocation of 4 d floats, which the reduction writes as one row
inline RowPlan row_plan_qk_bwd(long M, long d, bool qk_norm, bool contiguous, long ws_elems) {
  if (!qk_shape_ok(d)) return RowPlan{};
  const bool ws_form = qk_norm && contiguous;
  if (d >= 2048) {
    const long g = row_min(M, QK_BWD_GRID_BROW), lds = qk_norm ? 2 * d * (long)sizeof(float) : 0;
    if (ws_form && ws_elems >= g * 4 * d) return row_plan_ws(row_plan(BLOCK_ROW, d <= 2048 ? 1 : 2, g, 0, lds), 4 * d);
    return row_plan(BLOCK_ROW, d <= 2048 ? 1 : 2, qk_norm ? row_min(g, ROW_BROW_GRID_ATOMICS) : g, 0, lds);
  }
  const long wide = row_min(grid_rows(M), QK_BWD_GRID_WROW_WS), lds = qk_norm ? (2 * d + 4096) * (long)sizeof(float) : 0;
  if (ws_form && ws_elems >= wide * 4 * d && wide >= ROW_WS_MIN_GRID) return row_plan_ws(row_plan(WAVE_ROW, qk_nit(d), wide, 0, lds), 4 * d);
  return row_plan(WAVE_ROW, qk_nit(d), row_min(grid_rows(M), QK_BWD_GRID_WROW_ATOMICS), 0, lds);
}
