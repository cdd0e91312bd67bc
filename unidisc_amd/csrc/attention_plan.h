// Which device programs one udm_attention_fwd / udm_attention_bwd call runs, as a pure host function of the problem and the debug switches.  Plain C++17 without
// HIP: attention.hip executes the plan, tests/test_attention_plan.py compiles this header alone and prints the plan of every shape the GPU tests use.
//   forward   FWD_8WAVE (attn_fwd_kernel)      | FWD_GEN64 (attention_fwd64.hip)
//   dQ        DQ_8WAVE (attn_bwd_dq_kernel)    | DQ_GEN64 (attention_dq64.hip)
//   dK / dV   DKV_SINGLE (attn_bwd_dkv_kernel) | DKV_HALVES_D256 (its dK half, then its dV half) | DKV_WS / DKV_WS_PRE (attention_dkv_ws.hip, PRE: the score
//             chains start from the planes) | DKV_WS_SPLIT_SINGLE (packed documents: both, see below) | DKV_GEN64 (attention_dkv64.hip)
// The planes: delta | -lse | -delta, B H L floats each, in the caller's `delta` scratch.  DKV_GEN64 and the PRE kernel read them, so the dQ program that runs first
// must have written them: DQ_GEN64 always does, DQ_8WAVE does for pre-scaled q (attn_plan_bwd asserts that of the dQ program it chose).
#pragma once
#include <assert.h>
#include <stdint.h>

struct AttnProblem {
  int D, B, H, L;
  bool sample_ids, doc_ranges, causal, q_prescaled;
  bool dropout;   // attn_drop_thr(p_drop) > 0 (thr == 0 is the call without dropout: the same plan, the same kernels)
  long q_stride, k_stride, v_stride, o_stride, do_stride, out_stride, out2_stride, out3_stride;   // elements; out = O (forward) / dQ, out2 = dK, out3 = dV
};
// one field per debug key / environment variable (attention.hip owns the one instance); the defaults are those of an empty environment
struct AttnSwitches {
  int fwd64 = 1, dq64 = 1, dkv64 = 1;   // the generated programs: 0 off, 1 on, 2 on without the balanced walk
  int dkv_ws = 1;                       // 0: the single-role dK/dV kernel at head dim 128 too
  int dkv_pre = 1;                      // 0: the plain arithmetic of the wave-specialised kernel also for pre-scaled q
  int tr_read = 1;                      // 0: the kernels that gather transposed fragments with scalar LDS reads (USE_TR = false)
};
enum AttnFwdProgram { FWD_8WAVE, FWD_GEN64 };
enum AttnDqProgram { DQ_8WAVE, DQ_GEN64 };
enum AttnDkvProgram { DKV_SINGLE, DKV_HALVES_D256, DKV_WS, DKV_WS_PRE, DKV_WS_SPLIT_SINGLE, DKV_GEN64 };

// launch numbers of a generated (persistent) program: one workgroup per CU walks the 256-row blocks id, id + grid, ...
struct AttnGrid {
  uint32_t grid, nfull, hashalf;   // hashalf: blocks [0, nfull) are walked whole, the rest as 128-row halves (the balanced walk)
  uint32_t mg_nt, mg_H;            // magic divisors of L / 256 and H
};
struct AttnPlan {
  AttnFwdProgram fwd = FWD_8WAVE;
  AttnDqProgram dq = DQ_8WAVE;
  AttnDkvProgram dkv = DKV_SINGLE;
  bool planes_needed = false;   // the dK/dV program reads the planes: DKV_GEN64, DKV_WS_PRE, and DKV_WS_SPLIT_SINGLE when its wave-specialised half is the PRE form
  AttnGrid fwd_grid{}, dq_grid{}, dkv_grid{};   // of the FWD_GEN64 / DQ_GEN64 / DKV_GEN64 choices
};

// keep iff a 16-bit field >= thr (include/unidisc_hip.h); a p_drop that rounds to no step of the 65536 is no dropout
inline uint32_t attn_drop_thr(float p_drop) { return (uint32_t)(p_drop * 65536.0f + 0.5f); }

inline uint32_t attn_magic(long d) { return (uint32_t)((1ULL << 32) / (unsigned long long)d + 1); }   // n / d == mulhi(n, magic) for n d < 2^32, d >= 2 (magic(1) wraps)

// dev_cus: the device's CU count; plan_cus: udm_gemm_cus_available().  A persistent workgroup needs a whole CU: while a collective's channel kernels hold CUs
// (udm_gemm_set_cus, the data-parallel schedule `overlap_planned`) the grid is what is left - a workgroup that finds no CU would start its whole walk only when
// another has finished its own.
inline AttnGrid attn_persistent_grid(const AttnProblem& p, int sw, int dev_cus, int plan_cus) {
  dev_cus = dev_cus / 8 * 8;
  plan_cus = plan_cus / 8 * 8;
  const int cus = plan_cus >= 8 && plan_cus < dev_cus ? plan_cus : dev_cus;
  const long nt = p.L / 256, nblk = nt * p.B * p.H;
  const long grid = nblk < cus ? nblk : cus;
  // balanced walk: when the blocks left behind the whole rounds are exactly half a grid (the headline's 640 blocks on 256 CUs), every workgroup ends with ONE
  // 128-row half block (2.5 units each) instead of a third whole block for half of them (3 vs 2)
  const long rem = nblk % grid;
  const bool halves = sw != 2 && rem * 2 == grid && nblk - rem >= grid && grid % 16 == 0;
  return AttnGrid{(uint32_t)grid, (uint32_t)(halves ? nblk - rem : nblk), halves ? 1u : 0u, attn_magic(nt), attn_magic(p.H)};
}

// what the three generated programs ask alike: head dim 128 with the transposing reads, no mask of any kind, q pre-scaled, whole 256-row blocks with at least two
// trips of the tile loop, H >= 2 (magic(1) wraps: the head divisor would read 0), the XCD-sequential block order (B H a multiple of 8), 32-bit row / lse / plane
// indices and exact magic divisions
inline bool attn_gen64_shape(const AttnProblem& p, const AttnSwitches& sw) {
  if (p.D != 128 || p.sample_ids || !sw.tr_read || !p.q_prescaled || p.causal || p.dropout) return false;
  if (p.H < 2 || p.L % 256 != 0 || p.L < 512 || (p.B * p.H) % 8 != 0) return false;
  const long nt = p.L / 256, nblk = nt * p.B * p.H;
  return !((long)p.B * p.L >= (1L << 30) || nblk >= (1L << 24) || nt > 4096 || p.H > 4096 || (long)p.B * p.H * p.L >= (1L << 29));
}
// What each program asks of the strides on top of that: 16-byte row segments of what it stores or loads as whole rows, and 32-bit lane offsets over the rows one
// instruction spans.  The lists differ on purpose, each is its program's: the forward walks K / V 80 rows ahead and never checks q / k / v alignment (the entry
// point's % 8 check covers them); dQ spans 256 rows of q / dO / O / dQ and 64 of K / V; dK/dV the other way round.
inline bool attn_fwd64_takes(const AttnProblem& p, const AttnSwitches& sw) {
  const long lim = 1L << 31;
  if (!sw.fwd64 || !attn_gen64_shape(p, sw) || p.out_stride % 8 != 0) return false;
  return !(p.q_stride * 2 * 256 >= lim || p.k_stride * 2 * 80 >= lim || p.v_stride * 2 * 80 >= lim || p.out_stride * 2 * 256 >= lim);
}
inline bool attn_dq64_takes(const AttnProblem& p, const AttnSwitches& sw) {
  const long lim = 1L << 31;
  if (!sw.dq64 || !attn_gen64_shape(p, sw)) return false;
  if (p.out_stride % 8 != 0 || p.o_stride % 8 != 0 || p.q_stride % 8 != 0 || p.do_stride % 8 != 0) return false;
  return !(p.q_stride * 2 * 256 >= lim || p.do_stride * 2 * 256 >= lim || p.o_stride * 2 * 256 >= lim || p.k_stride * 2 * 64 >= lim || p.v_stride * 2 * 64 >= lim ||
           p.out_stride * 2 * 256 >= lim);
}
inline bool attn_dkv64_takes(const AttnProblem& p, const AttnSwitches& sw) {
  const long lim = 1L << 31;
  if (!sw.dkv64 || !attn_gen64_shape(p, sw)) return false;
  if (p.out2_stride % 8 != 0 || p.out3_stride % 8 != 0 || p.q_stride % 8 != 0 || p.do_stride % 8 != 0) return false;
  return !(p.q_stride * 2 * 64 >= lim || p.do_stride * 2 * 64 >= lim || p.k_stride * 2 * 256 >= lim || p.v_stride * 2 * 256 >= lim || p.out2_stride * 2 * 256 >= lim ||
           p.out3_stride * 2 * 256 >= lim);
}

inline AttnPlan attn_plan_fwd(const AttnProblem& p, const AttnSwitches& sw, int dev_cus, int plan_cus) {
  AttnPlan plan;
  if (attn_fwd64_takes(p, sw)) { plan.fwd = FWD_GEN64; plan.fwd_grid = attn_persistent_grid(p, sw.fwd64, dev_cus, plan_cus); }
  return plan;
}

inline AttnPlan attn_plan_bwd(const AttnProblem& p, const AttnSwitches& sw, int dev_cus, int plan_cus) {
  AttnPlan plan;
  if (attn_dq64_takes(p, sw)) { plan.dq = DQ_GEN64; plan.dq_grid = attn_persistent_grid(p, sw.dq64, dev_cus, plan_cus); }
  // Head dim 128: both accumulators (128 registers) plus K/V operands (64) only fit one wave per SIMD in the single-role kernel, which is then bound by that one
  // wave's instruction issue (0.39 ms at B8 H16 L1280); without a mask the wave-specialised kernel (0.27 ms) or the generated program runs instead.  Neither has a
  // causal, dropout or USE_TR = false form.  Head dim 256: dK^T and dV^T together are more registers than a wave has - the dK half, then the dV half.
  const bool d128 = p.D == 128 && sw.tr_read && !p.causal && !p.dropout;
  const bool pre = p.q_prescaled && sw.dkv_pre;   // the wave-specialised kernel's score chains start from -lse / -delta
  if (p.D == 256) plan.dkv = DKV_HALVES_D256;
  else if (attn_dkv64_takes(p, sw)) { plan.dkv = DKV_GEN64; plan.dkv_grid = attn_persistent_grid(p, sw.dkv64, dev_cus, plan_cus); }
  else if (d128 && !p.sample_ids && sw.dkv_ws) plan.dkv = pre ? DKV_WS_PRE : DKV_WS;
  // packed documents: key blocks that lie inside one document and whose query span is exactly that document go to the wave-specialised kernel (no id test
  // needed anywhere); the blocks at document boundaries / with padding stay with the single-role kernel
  else if (d128 && p.sample_ids && p.doc_ranges && sw.dkv_ws) plan.dkv = DKV_WS_SPLIT_SINGLE;
  plan.planes_needed = plan.dkv == DKV_GEN64 || plan.dkv == DKV_WS_PRE || (plan.dkv == DKV_WS_SPLIT_SINGLE && pre);
  // what the chosen dQ program writes, not what the readers' gates happen to ask: a planes reader chosen for plain q while the 8-wave dQ kernel runs aborts here
  // (and in tests/test_attention_plan.py, whose printer is built with assertions on and asks for every reader's shape with plain q)
  assert(!plan.planes_needed || plan.dq == DQ_GEN64 || (plan.dq == DQ_8WAVE && p.q_prescaled));
  return plan;
}

// ---- the rectangular forward (attention_kv.hip, udm_attention_fwd_kv): Lq queries against Lk cached keys, inference only --------------------------------------
// One program: the 8-wave body at 128 queries per workgroup and 64-key tiles, instantiated per head dim, always with the transposing LDS reads.  No key
// split: the grid is ceil(Lq / 128) B H workgroups whatever Lk is (256 at B 8, H 16, Lq 256; 32 at B 1 - DESIGN.md "Modality KV cache" has the prices).
// Workgroups per CU the kernel is compiled for (the square forward's numbers: at head dim 256 the four 32 KiB stages and 128 + 64 registers of O^T and Q leave
// room for one).
constexpr int ATTN_KV_WGS(int D) { return D == 256 ? 1 : 2; }
struct AttnKvProblem {
  int D;
  long B, H, Lq, Lk;
};
struct AttnKvPlan {
  int D = 0;
  uint32_t q_tiles = 0;     // 128-query blocks per (b, h)
  uint32_t kv_tiles = 0;    // 64-key tiles every block walks
  uint32_t grid = 0;        // q_tiles * B * H workgroups of 256 threads
  uint32_t lds_bytes = 0;   // K0 | K1 | V0 | V1
  bool grid_ok = false;     // the grid fits 31 bits
};
inline AttnKvPlan attn_plan_fwd_kv(const AttnKvProblem& p) {
  AttnKvPlan plan;
  plan.D = p.D;
  const long qt = (p.Lq + 127) / 128, grid = qt * p.B * p.H;
  plan.grid_ok = grid > 0 && grid < (1L << 31);
  plan.q_tiles = (uint32_t)qt;
  plan.kv_tiles = (uint32_t)((p.Lk + 63) / 64);
  plan.grid = plan.grid_ok ? (uint32_t)grid : 0;
  plan.lds_bytes = (uint32_t)(4 * 64 * p.D * 2);
  return plan;
}

// ---- the causal form (attention_kv.hip, udm_attention_fwd_kv_causal): query i sees the keys j <= i + (Lk - Lq), the queries being the LAST Lq positions
// (Lk >= Lq; chunked prefill over a K / V cache).  The plan is attn_plan_fwd_kv's; what differs is where a workgroup's walk ends: the 128-query block
// `q_tile` walks the 64-key tiles [0, end) with end = ceil((min(128 (q_tile + 1), Lq) + Lk - Lq) / 64) - the tiles that hold a key visible to its LAST live query.
// Every visible key of the block lies in a walked tile and the last walked tile holds one (tests/test_attention_kv_causal_plan.py, against brute force).
// constexpr: the kernel calls it too.
constexpr long attn_kv_causal_walk_end(long Lq, long Lk, long q_tile) {
  const long q_end = 128 * (q_tile + 1) < Lq ? 128 * (q_tile + 1) : Lq;
  return (q_end + (Lk - Lq) + 63) / 64;
}

// ---- the key-split form (attention_kv.hip, udm_attention_fwd_kv_split): the same body, S workgroups per (128-query block, b, h), each over a contiguous range
// of 64-key tiles; fp32 partials (m, l, unnormalised O) per query row in a workspace, a second launch combines them in the fixed order s = 0 .. S - 1.
// The consumer is the conditioning K / V cache at batch 1 or 2 (DESIGN.md "Conditioning K/V cache"): 256 queries against 1280 keys are 32 workgroups unsplit.
constexpr int ATTN_KV_MAX_SPLITS = 32;
struct AttnKvSplitPlan {
  AttnKvPlan base;          // the unsplit plan of the same problem (q_tiles, kv_tiles, lds_bytes); S = 1 launches exactly it
  uint32_t splits = 1;      // S
  uint32_t grid = 0;        // q_tiles * B * H * S workgroups
  long ws_elems = 0;        // floats the workspace must hold for S splits: S B H Lq (D + 2), 0 for S = 1
  bool grid_ok = false;
};
// floats of workspace S splits need: per (split, b, h, query row) the D unnormalised outputs, then m and l.  Layout: all O rows ([S][B][H][Lq][D]), then all
// (m, l) pairs ([S][B][H][Lq][2]) - 16-byte rows for the kernels' four-float stores.
inline long attn_kv_split_ws_elems(const AttnKvProblem& p, long S) { return S <= 1 ? 0 : S * p.B * p.H * p.Lq * (long)(p.D + 2); }
// tiles [begin, end) of split s: balanced, the first kv_tiles % S splits take one more (9 tiles in 4 splits: 3, 2, 2, 2); the last range carries the Lk tail
inline void attn_kv_split_range(long kv_tiles, long S, long s, long& begin, long& end) {
  const long base = kv_tiles / S, rem = kv_tiles % S;
  begin = s * base + (s < rem ? s : rem);
  end = begin + base + (s < rem ? 1 : 0);
}
// a requested split count lowered to what can run: every split owns at least one key tile, at most ATTN_KV_MAX_SPLITS, and what `ws_elems` floats hold
// (have_ws = false: the NULL workspace, one split)
inline long attn_kv_split_clamp(const AttnKvProblem& p, long S, bool have_ws, long ws_elems) {
  const long T = (p.Lk + 63) / 64, per = p.B * p.H * p.Lq * (long)(p.D + 2);
  if (S > T) S = T;
  if (S > ATTN_KV_MAX_SPLITS) S = ATTN_KV_MAX_SPLITS;
  if (!have_ws) S = 1;
  else if (per > 0 && S > ws_elems / per) S = ws_elems / per;
  return S < 1 ? 1 : S;
}
inline AttnKvSplitPlan attn_kv_split_with(const AttnKvProblem& p, long S) {
  AttnKvSplitPlan plan;
  plan.base = attn_plan_fwd_kv(p);
  const long grid = (long)plan.base.grid * S;
  plan.grid_ok = plan.base.grid_ok && grid < (1L << 31);
  plan.splits = (uint32_t)S;
  plan.grid = plan.grid_ok ? (uint32_t)grid : 0;
  plan.ws_elems = attn_kv_split_ws_elems(p, S);
  return plan;
}
// The plan's own choice (splits = 0).  One split while the unsplit grid fills at least a QUARTER of the device's workgroup slots (ATTN_KV_WGS per CU): the second
// launch and the fp32 round trip of the partials then cost more than the idle CUs win.  Otherwise the smallest power of two that brings the grid to HALF the
// slots - one workgroup per CU at head dim <= 128 - halved until every split keeps at least two key tiles (and at most ATTN_KV_MAX_SPLITS).
// Both fractions are measured (RESULTS.md "Conditioning K/V cache", 256 CUs, H 16, D 128, Lk 1280): the first form of this rule - split below half of the slots,
// up to all of them - chose S = 4 at Lq 1024, B 1 (128 workgroups, a quarter of the slots), 4 % slower than unsplit, and S = 8 at Lq 256, B 2, where S = 4 is
// 17 % faster than S = 8.  At Lq 256, B 1 both forms give S = 8 (0.69 of the unsplit time).
inline AttnKvSplitPlan attn_plan_fwd_kv_split(const AttnKvProblem& p, int dev_cus) {
  const AttnKvPlan base = attn_plan_fwd_kv(p);
  const long slots = (long)dev_cus * ATTN_KV_WGS(p.D), T = base.kv_tiles;
  long S = 1;
  if (base.grid_ok && 4L * base.grid < slots) {
    while (2L * base.grid * S < slots && S < ATTN_KV_MAX_SPLITS) S *= 2;
    while (S > 1 && T / S < 2) S /= 2;
  }
  return attn_kv_split_with(p, S);
}
