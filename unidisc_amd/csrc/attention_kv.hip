// Rectangular flash attention forward (inference only): Lq queries against Lk keys / values that live in another buffer - a per-layer K / V cache.
//   o[b, i, h, :] = softmax_j(q[b, i, h] . k[b, j, h]) v[b, j, h],  0 <= i < Lq, 0 <= j < Lk
// The consumer: the text steps of `eval.attention_caching` with eval.attention_caching_read_cache (text queries against [fresh text keys ; cached image
// keys], the reference's stated intent at models/dit.py:790-792).  udm_attention_fwd_kv and its split form are bidirectional; the causal form is an entry of
// its own, udm_attention_fwd_kv_causal (below).
//
// The body is the 8-wave forward of attention.hip (attn_fwd_kernel) without sample ids and dropout: 128 queries per workgroup (4 waves x 32), 64-key tiles,
// S^T = K Q^T so that a lane owns one query column and the softmax state is lane-local, K / V tiles by LDS-DMA into two XOR-swizzled stages each, the lazy
// reference exponent, whole-row O stores through the idle stages at head dim 128.  What differs is the addressing - every operand has its own row AND batch
// stride (element (b, l, h, :) at base + b batch + l stride + h D), queries are bounded by Lq and keys by Lk.
// The kernel only reads k and v: appending the current rows' keys is the caller's copy (a fused append would make one workgroup read
// rows another one writes).  Key rows >= Lk are never addressed (an overhanging tile re-reads row Lk - 1 and masks it), query rows >= Lq neither.
// udm_attention_fwd_kv_split is the same body with the keys split over S workgroups per (query block, b, h) and a combine launch: the read steps of the
// conditioning K / V cache (`eval.conditioning_cache`) run at batch 1 or 2, where the unsplit grid leaves most CUs idle.
// udm_attention_fwd_kv_causal is the same body under the rectangular causal mask: query i sees the keys j <= i + (Lk - Lq), the queries being the LAST Lq
// positions (Lk >= Lq).  The consumer: the chunked cached forward of the AR baseline (DIT._forward_chunk: n tokens at cache slots [p, p + n) against the keys
// [0, p + n)).  A workgroup walks key tiles only up to the frontier of its last live query (attn_kv_causal_walk_end, attention_plan.h), and only a tile that
// crosses the frontier of one of a wave's 32 queries takes the per-element test.  Key 0 is visible to every query, so no row is ever dead.  No split form.
#include "attention_common.h"
#include <type_traits>

namespace {

constexpr int BQ = 128;   // query rows per block (4 waves x 32)
constexpr int BKV = 64;   // keys per tile

// its own argument block: AttnArgs is full and its layout is shared with the generated programs
struct AttnKvArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v;
  bf16_t* out;
  float* lse;           // [B, H, Lq] log2-domain log-sum-exp of the scaled scores, or null
  long q_stride, k_stride, v_stride, o_stride;   // row strides, elements
  long q_batch, k_batch, v_batch, o_batch;       // batch strides, elements
  int B, H, Lq, Lk;
  float scale_log2;     // log2(e) / sqrt(D); 1 for pre-scaled q
};

// SPLIT (udm_attention_fwd_kv_split): the workgroup walks the key tiles of ONE of S contiguous ranges and leaves its softmax state - the reference exponent m c,
// the row sum l and the unnormalised O - in fp32 in `ws` instead of dividing and storing O; attn_kv_combine_kernel folds the S partials of a row.
// CAUSAL (udm_attention_fwd_kv_causal): the walk ends at the block's frontier and the tiles that cross a wave's frontier are masked per element.
template <int D, bool SPLIT, bool CAUSAL = false>
__device__ __forceinline__ void attn_fwd_kv_body(const AttnKvArgs& a, float* ws, int S) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // K0 | K1 | V0 | V1   (one array: keeps LDS-DMA waits exact)
  constexpr int TB = BKV * D * 2;
  constexpr int KS = D / 16, DB = D / 32;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, tile_x, split = 0;
  attn_block_to_work(blockIdx.x, a.B * a.H, bh, tile_x);   // all query tiles of one (b, h) on one XCD: they share its K / V through that L2
  if constexpr (SPLIT) {   // (query tile, split) pairs take the place of the query tiles: the query tiles of one split are adjacent (they walk the same keys)
    const int q_tiles = (a.Lq + BQ - 1) / BQ;
    split = tile_x / q_tiles;
    tile_x -= split * q_tiles;
  }
  const int b = bh / a.H, h = bh % a.H;
  const int qi = tile_x * BQ + wave * 32 + l31;
  const bool q_ok = qi < a.Lq;

  bf16x8_t qf[KS];
  const bf16_t* qrow = a.q + (long)b * a.q_batch + (long)qi * a.q_stride + h * D + hi * 8;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = load_frag_global(qrow + ks * 16, q_ok);
  // (as in attn_fwd_kernel: the compiler's wait for these loads must land before the loop, whose only outstanding vector-memory operations are the
  // inline-asm LDS-DMA refills it must not wait for)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));

  f32x16_t oT[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oT[i][r] = 0.f;
  float m = -INFINITY, lsum = 0.f;
  const float c = a.scale_log2;

  const bf16_t* kbase = a.k + (long)b * a.k_batch + h * D;
  const bf16_t* vbase = a.v + (long)b * a.v_batch + h * D;
  using Stg = DmaStager<D, BKV>;
  DmaPlan<D, BKV> plank, planv;
  plank.init(a.k_stride, wave, lane);
  planv.init(a.v_stride, wave, lane);
  int t_begin = 0, t_end = (a.Lk + BKV - 1) / BKV;
  // causal: the last key query qi sees, and the first key some query of this wave does NOT see (wave-uniform: tiles that end before it need no test)
  const int off = a.Lk - a.Lq, k_last = qi + off;
  const int wave_front = tile_x * BQ + wave * 32 + off + 1;
  if constexpr (CAUSAL) t_end = (int)attn_kv_causal_walk_end(a.Lq, a.Lk, tile_x);   // (the staging below is bounded by a.Lk and t_end, whichever tile the walk ends at)
  if constexpr (SPLIT) {   // attn_kv_split_range (attention_plan.h): S <= tiles, so no range is empty
    const int base = t_end / S, rem = t_end % S;
    t_begin = split * base + min(split, rem);
    t_end = t_begin + base + (split < rem ? 1 : 0);
  }
  Stg::issue(kbase, a.k_stride, t_begin * BKV, a.Lk, smem, wave, lane);            // (rows past Lk - 1 are clamped to it: no key row >= Lk is ever addressed)
  Stg::issue(vbase, a.v_stride, t_begin * BKV, a.Lk, smem + 2 * TB, wave, lane);
  auto tile = [&](auto st_c, int t) {   // the stage as a compile-time constant: fragment addresses are a hoisted per-lane register plus an immediate
    constexpr int st = decltype(st_c)::value;
    const int kv0 = t * BKV;
    const char* Ks = smem + st * TB;
    const char* Vs = smem + (2 + st) * TB;
    wait_all_vmem();   // this wave's share of tile t has landed
    __syncthreads();   // ... and everybody's; all waves are also done with tile t-1, so its stage may be refilled
    if (t + 1 >= t_end) {
    } else if (kv0 + 2 * BKV <= a.Lk) {   // the next tile is a full one: offsets are precomputed, the tile base is wave-uniform
      plank.issue_full(kbase + (long)(kv0 + BKV) * a.k_stride, smem + (st ^ 1) * TB, wave);
      planv.issue_full(vbase + (long)(kv0 + BKV) * a.v_stride, smem + (2 + (st ^ 1)) * TB, wave);
    } else {
      Stg::issue(kbase, a.k_stride, kv0 + BKV, a.Lk, smem + (st ^ 1) * TB, wave, lane);
      Stg::issue(vbase, a.v_stride, kv0 + BKV, a.Lk, smem + (2 + (st ^ 1)) * TB, wave, lane);
    }
    // S^T = K Q^T : [64 keys] x [32 queries per wave]; two alternating 32-key chains, K fragments read two k-steps ahead of their MFMAs
    f32x16_t sT[2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) sT[f][r] = 0.f;
    {
      bf16x8_t kq[3][2];
#pragma unroll
      for (int pre = 0; pre < 2; ++pre)
#pragma unroll
        for (int f = 0; f < 2; ++f) kq[pre][f] = lds_frag(Ks, tile_off<D>(f * 32 + l31, pre * 2 + hi));
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + 2 < KS) {
#pragma unroll
          for (int f = 0; f < 2; ++f) kq[(ks + 2) % 3][f] = lds_frag(Ks, tile_off<D>(f * 32 + l31, (ks + 2) * 2 + hi));
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) sT[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kq[ks % 3][f], qf[ks], sT[f], 0, 0, 0);
      }
    }
    // Causal: mvote is the tile maximum BEFORE the causal mask (after the ragged one): the wave votes on it (below), so it takes the rescale branch exactly
    // where the bidirectional kernel does, and a query that sees every key - the last one - goes through the same arithmetic bit for bit.  What a lane moves
    // its exponent TO is the maximum of the keys it sees.
    float mvote = -INFINITY;
    if constexpr (CAUSAL) {
      // ONE wave-uniform branch per tile, as in the bidirectional body: the tile overhangs Lk, or crosses the frontier of one of this wave's queries.
      // Element (f, r) is key kv0 + 4 hi + a compile-time constant, so each test is that constant against one per-lane value of the tile.
      if (kv0 + BKV > min(wave_front, a.Lk)) {
        const int rel_lk = a.Lk - 1 - kv0 - 4 * hi, rel = min(k_last, a.Lk - 1) - kv0 - 4 * hi;
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kc = f * 32 + (r & 3) + 8 * (r >> 2);
            const float s_lk = kc > rel_lk ? -INFINITY : sT[f][r];   // the ragged mask: what the bidirectional kernel's maximum is taken over
            mvote = fmaxf(mvote, s_lk);
            sT[f][r] = kc > rel ? -INFINITY : s_lk;
          }
        mvote = fmaxf(mvote, __shfl_xor(mvote, 32, 64));
      }
    } else if (kv0 + BKV > a.Lk) {   // the ragged last tile (before the running maximum: a masked score contributes exp2(-inf) = 0 exactly)
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kl = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kv0 + kl >= a.Lk) sT[f][r] = -INFINITY;
        }
    }
    float p[2][16];
    float mloc = -INFINITY;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, sT[f][r]);
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    if constexpr (CAUSAL) mvote = fmaxf(mvote, mloc);   // (a tile without a test: the maximum itself; with one: the unmasked maximum is the larger)
    // Lazy rescale (attn_fwd_kernel): m is the REFERENCE exponent of this query, moved only when some query of the wave saw a score more than 2^8 above it.
    const bool move = q_ok && ((CAUSAL ? mvote : mloc) * c > m * c + 8.0f);   // (lanes of query rows past Lq never vote)
    if (__builtin_amdgcn_ballot_w64(move) != 0) {
      const float m_new = fmaxf(m, mloc);
      const float alpha = __builtin_amdgcn_exp2f((m - ((m_new == -INFINITY) ? 0.f : m_new)) * c);
      lsum *= alpha;
      m = m_new;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oT[i][r] *= alpha;
    }
    const float mc = (m == -INFINITY) ? 0.f : m * c;
    float psum = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[f][r] = __builtin_amdgcn_exp2f(sT[f][r] * c - mc);
        psum += p[f][r];
      }
    lsum += psum;
    // O^T += V^T P^T
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      bf16x8_t pb = pack8(&p[cc >> 1][8 * (cc & 1)]);
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        bf16x8_t vt = lds_frag_T<D, true>(Vs, cc * 16, i * 32, lane);
        oT[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, pb, oT[i], 0, 0, 0);
      }
    }
  };
  {
    int t = t_begin;
    for (; t + 1 < t_end; t += 2) {
      tile(std::integral_constant<int, 0>{}, t);
      tile(std::integral_constant<int, 1>{}, t + 1);
    }
    if (t < t_end) tile(std::integral_constant<int, 0>{}, t);
  }
  const float ltot = lsum + __shfl_xor(lsum, 32, 64);
  if constexpr (SPLIT) {
    // partials of row (split, b, h, qi): D floats of O^T as the lane holds them (four consecutive columns per store), then (m c, l) - m c is the row's reference
    // exponent in base-2 units (-inf: nothing accumulated), the scale every p = 2^(s c - m c) of this split was taken against
    if (q_ok) {
      const long rows = (long)a.B * a.H * a.Lq, row = ((long)split * a.B * a.H + bh) * a.Lq + qi;
      float* op = ws + row * D;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg)
          *reinterpret_cast<float4*>(op + i * 32 + 8 * rg + 4 * hi) = make_float4(oT[i][rg * 4], oT[i][rg * 4 + 1], oT[i][rg * 4 + 2], oT[i][rg * 4 + 3]);
      if (hi == 0) *reinterpret_cast<float2*>(ws + (long)S * rows * D + row * 2) = make_float2(m == -INFINITY ? -INFINITY : m * c, ltot);
    }
    return;
  }
  const float inv = ltot > 0.f ? 1.f / ltot : 0.f;
  if (a.lse != nullptr && q_ok && hi == 0) a.lse[((long)b * a.H + h) * a.Lq + qi] = ltot > 0.f ? __builtin_fmaf(m, c, log2f(ltot)) : INFINITY;
  bf16_t* obase = a.out + (long)b * a.o_batch + h * D;
  if constexpr (D == 128) {   // whole-row stores through the (now idle) K / V stages; o_stride % 8 == 0 is an argument check of the entry point
    __syncthreads();
    const int q0 = tile_x * BQ + wave * 32;
    store_rows_via_lds_d128(smem + wave * 8192, oT, inv, obase + (long)q0 * a.o_stride, a.o_stride, a.Lq - q0, lane);
  } else {
    if (q_ok) {
      bf16_t* op = obase + (long)qi * a.o_stride;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int d0 = i * 32 + 8 * rg + 4 * hi;
          *reinterpret_cast<uint2*>(op + d0) = make_uint2(pack2bf(oT[i][rg * 4] * inv, oT[i][rg * 4 + 1] * inv), pack2bf(oT[i][rg * 4 + 2] * inv, oT[i][rg * 4 + 3] * inv));
        }
    }
  }
}

template <int D>
__global__ __launch_bounds__(256, ATTN_KV_WGS(D)) void attn_fwd_kv_kernel(AttnKvArgs a) { attn_fwd_kv_body<D, false>(a, nullptr, 1); }
template <int D>
__global__ __launch_bounds__(256, ATTN_KV_WGS(D)) void attn_fwd_kv_split_kernel(AttnKvArgs a, float* ws, int S) { attn_fwd_kv_body<D, true>(a, ws, S); }
template <int D>
__global__ __launch_bounds__(256, ATTN_KV_WGS(D)) void attn_fwd_kv_causal_kernel(AttnKvArgs a) { attn_fwd_kv_body<D, false, true>(a, nullptr, 1); }

// The S partials of a query row, folded in the fixed order s = 0 .. S - 1 (no atomics: the same bits on every launch): M = max_s m_s,
// O = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s, one rounding to bf16; lse2 = M + log2 of that denominator.  One thread per (row, four columns).
template <int D>
__global__ __launch_bounds__(256) void attn_kv_combine_kernel(AttnKvArgs a, const float* ws, int S) {
  constexpr int CH = D / 4;                       // threads per row
  const long rows = (long)a.B * a.H * a.Lq;
  const long row = (long)blockIdx.x * (256 / CH) + threadIdx.x / CH;
  const int ch = threadIdx.x % CH;
  if (row >= rows) return;
  const float* ml = ws + (long)S * rows * D;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, ml[((long)s * rows + row) * 2]);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float l = 0.f;
  for (int s = 0; s < S; ++s) {
    const float2 p = *reinterpret_cast<const float2*>(ml + ((long)s * rows + row) * 2);
    const float w = p.x == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(p.x - M);
    const float4 o = *reinterpret_cast<const float4*>(ws + ((long)s * rows + row) * D + ch * 4);
    acc.x = __builtin_fmaf(w, o.x, acc.x); acc.y = __builtin_fmaf(w, o.y, acc.y); acc.z = __builtin_fmaf(w, o.z, acc.z); acc.w = __builtin_fmaf(w, o.w, acc.w);
    l = __builtin_fmaf(w, p.y, l);
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  const int qi = (int)(row % a.Lq);
  const long bh = row / a.Lq;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  bf16_t* op = a.out + (long)b * a.o_batch + (long)qi * a.o_stride + h * D + ch * 4;
  *reinterpret_cast<uint2*>(op) = make_uint2(pack2bf(acc.x * inv, acc.y * inv), pack2bf(acc.z * inv, acc.w * inv));
  if (a.lse != nullptr && ch == 0) a.lse[row] = l > 0.f ? M + log2f(l) : INFINITY;
}

template <int D>
void launch_kv_split(const AttnKvSplitPlan& plan, const AttnKvArgs& a, float* ws, hipStream_t s) {
  static bool once = false;
  if (!once) { (void)hipFuncSetAttribute((const void*)attn_fwd_kv_split_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.base.lds_bytes); once = true; }
  const int S = (int)plan.splits;
  hipLaunchKernelGGL((attn_fwd_kv_split_kernel<D>), dim3(plan.grid), dim3(256), plan.base.lds_bytes, s, a, ws, S);
  const long rows = (long)a.B * a.H * a.Lq, per = 256 / (D / 4);
  hipLaunchKernelGGL((attn_kv_combine_kernel<D>), dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, s, a, (const float*)ws, S);
}

template <int D>
void launch_kv(const AttnKvPlan& plan, const AttnKvArgs& a, hipStream_t s) {
  static bool once = false;
  if (!once) { (void)hipFuncSetAttribute((const void*)attn_fwd_kv_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes); once = true; }
  hipLaunchKernelGGL((attn_fwd_kv_kernel<D>), dim3(plan.grid), dim3(256), plan.lds_bytes, s, a);
}

template <int D>
void launch_kv_causal(const AttnKvPlan& plan, const AttnKvArgs& a, hipStream_t s) {
  static bool once = false;
  if (!once) { (void)hipFuncSetAttribute((const void*)attn_fwd_kv_causal_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes); once = true; }
  hipLaunchKernelGGL((attn_fwd_kv_causal_kernel<D>), dim3(plan.grid), dim3(256), plan.lds_bytes, s, a);
}
}  // namespace

namespace {
int kv_device_cus() {
  static const int n = [] { int dev = 0, cus = 256; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); return cus; }();
  return n;
}

// all three entry points: the argument checks, then the unsplit launch (split_form = false, or a split count that came down to 1), the split pair, or the
// causal kernel (causal_form; never with split_form)
int kv_entry(const char* name, bool split_form, bool causal_form, const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D,
             int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t q_batch, int64_t k_batch, int64_t v_batch, int64_t o_batch, float* ws,
             int64_t ws_elems, int64_t splits, int64_t flags, hipStream_t stream) {
  UDM_CHECK_ARG(q && k && v && o, "%s: null pointer", name);
  UDM_CHECK_ARG((flags & ~(int64_t)UDM_ATTN_Q_PRESCALED) == 0, "%s: unknown flags %ld (UDM_ATTN_Q_PRESCALED only: the causal form is udm_attention_fwd_kv_causal)", name,
                (long)flags);
  UDM_CHECK_ARG(B > 0 && H > 0, "%s: empty problem", name);
  UDM_CHECK_ARG(Lq >= 1 && Lk >= 1, "%s: Lq = %ld, Lk = %ld (both >= 1)", name, (long)Lq, (long)Lk);
  UDM_CHECK_ARG(!causal_form || Lk >= Lq, "%s: Lk = %ld < Lq = %ld (the queries are the last Lq of the Lk positions)", name, (long)Lk, (long)Lq);
  UDM_CHECK_ARG(D == 32 || D == 64 || D == 128 || D == 256, "%s: head_dim %ld unsupported (32, 64, 128, 256)", name, (long)D);
  UDM_CHECK_ARG(q_stride % 8 == 0 && k_stride % 8 == 0 && v_stride % 8 == 0 && o_stride % 8 == 0, "%s: row strides must be multiples of 8 elements", name);
  UDM_CHECK_ARG(q_batch % 8 == 0 && k_batch % 8 == 0 && v_batch % 8 == 0 && o_batch % 8 == 0, "%s: batch strides must be multiples of 8 elements", name);
  UDM_CHECK_ARG(q_stride >= H * D && k_stride >= H * D && v_stride >= H * D && o_stride >= H * D && q_batch >= 0 && k_batch >= 0 && v_batch >= 0 && o_batch >= 0,
                "%s: a row stride below H * D, or a negative batch stride", name);
  UDM_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "%s: operand bases must be 16-byte aligned", name);
  // 32-bit lane offsets over the 64 rows one LDS-DMA tile spans; int shapes
  UDM_CHECK_ARG(Lq < (1LL << 30) && Lk < (1LL << 30) && B * H < (1LL << 30) && k_stride * 2 * 64 < (1LL << 31) && v_stride * 2 * 64 < (1LL << 31),
                "%s: shape or stride too large", name);
  const AttnKvProblem prob{(int)D, B, H, Lq, Lk};
  const AttnKvPlan plan = attn_plan_fwd_kv(prob);
  UDM_CHECK_ARG(plan.grid_ok, "%s: grid too large", name);
  AttnKvSplitPlan splan{};
  if (split_form) {
    UDM_CHECK_ARG(splits >= 0 && ws_elems >= 0, "%s: splits = %ld, ws_elems = %ld (both >= 0; splits = 0: the plan decides)", name, (long)splits, (long)ws_elems);
    UDM_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: ws must be 16-byte aligned", name);
    UDM_CHECK_ARG(B * H * Lq < (1LL << 31), "%s: shape or stride too large", name);
    const long want = splits > 0 ? (long)splits : (long)attn_plan_fwd_kv_split(prob, kv_device_cus()).splits;
    splan = attn_kv_split_with(prob, attn_kv_split_clamp(prob, want, ws != nullptr, (long)ws_elems));
    UDM_CHECK_ARG(splan.grid_ok, "%s: grid too large", name);
  }
  AttnKvArgs a{};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.out = (bf16_t*)o; a.lse = lse;
  a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride; a.o_stride = o_stride;
  a.q_batch = q_batch; a.k_batch = k_batch; a.v_batch = v_batch; a.o_batch = o_batch;
  a.B = (int)B; a.H = (int)H; a.Lq = (int)Lq; a.Lk = (int)Lk;
  a.scale_log2 = (flags & UDM_ATTN_Q_PRESCALED) ? 1.0f : (1.0f / sqrtf((float)D)) * 1.4426950408889634f;   // pre-scaled q: the scores ARE the base-2 exponents
  if (split_form && splan.splits > 1) {
    switch (plan.D) {
      case 256: launch_kv_split<256>(splan, a, ws, stream); break;
      case 128: launch_kv_split<128>(splan, a, ws, stream); break;
      case 64: launch_kv_split<64>(splan, a, ws, stream); break;
      default: launch_kv_split<32>(splan, a, ws, stream); break;
    }
    UDM_CHECK_LAUNCH(name);
    return 0;
  }
  if (causal_form) {
    switch (plan.D) {
      case 256: launch_kv_causal<256>(plan, a, stream); break;
      case 128: launch_kv_causal<128>(plan, a, stream); break;
      case 64: launch_kv_causal<64>(plan, a, stream); break;
      default: launch_kv_causal<32>(plan, a, stream); break;
    }
    UDM_CHECK_LAUNCH(name);
    return 0;
  }
  switch (plan.D) {
    case 256: launch_kv<256>(plan, a, stream); break;
    case 128: launch_kv<128>(plan, a, stream); break;
    case 64: launch_kv<64>(plan, a, stream); break;
    default: launch_kv<32>(plan, a, stream); break;
  }
  UDM_CHECK_LAUNCH(name);
  return 0;
}
}  // namespace

extern "C" int udm_attention_fwd_kv(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D, int64_t q_stride,
                                    int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t q_batch, int64_t k_batch, int64_t v_batch, int64_t o_batch, int64_t flags,
                                    hipStream_t stream) {
  return kv_entry("udm_attention_fwd_kv", false, false, q, k, v, o, lse, B, H, Lq, Lk, D, q_stride, k_stride, v_stride, o_stride, q_batch, k_batch, v_batch, o_batch, nullptr, 0, 1,
                  flags, stream);
}

extern "C" int udm_attention_fwd_kv_split(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D,
                                          int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t q_batch, int64_t k_batch, int64_t v_batch,
                                          int64_t o_batch, float* ws, int64_t ws_elems, int64_t splits, int64_t flags, hipStream_t stream) {
  return kv_entry("udm_attention_fwd_kv_split", true, false, q, k, v, o, lse, B, H, Lq, Lk, D, q_stride, k_stride, v_stride, o_stride, q_batch, k_batch, v_batch, o_batch, ws,
                  ws_elems, splits, flags, stream);
}

extern "C" int udm_attention_fwd_kv_causal(const void* q, const void* k, const void* v, void* o, float* lse, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D,
                                           int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride, int64_t q_batch, int64_t k_batch, int64_t v_batch,
                                           int64_t o_batch, int64_t flags, hipStream_t stream) {
  return kv_entry("udm_attention_fwd_kv_causal", false, true, q, k, v, o, lse, B, H, Lq, Lk, D, q_stride, k_stride, v_stride, o_stride, q_batch, k_batch, v_batch, o_batch,
                  nullptr, 0, 1, flags, stream);
}

extern "C" int udm_attention_kv_split_plan(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D, int64_t splits, int64_t* splits_out, int64_t* ws_elems_out) {
  const char* name = "udm_attention_kv_split_plan";
  UDM_CHECK_ARG(B > 0 && H > 0 && Lq >= 1 && Lk >= 1 && splits >= 0, "%s: empty problem or negative splits", name);
  UDM_CHECK_ARG(D == 32 || D == 64 || D == 128 || D == 256, "%s: head_dim %ld unsupported (32, 64, 128, 256)", name, (long)D);
  const AttnKvProblem prob{(int)D, B, H, Lq, Lk};
  const long want = splits > 0 ? (long)splits : (long)attn_plan_fwd_kv_split(prob, kv_device_cus()).splits;
  const long S = attn_kv_split_clamp(prob, want, true, INT64_MAX);
  if (splits_out) *splits_out = S;
  if (ws_elems_out) *ws_elems_out = attn_kv_split_ws_elems(prob, S);
  return 0;
}
