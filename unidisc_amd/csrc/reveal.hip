// The second half of a maskgit / maskgit_nucleus / first_hitting sampler step in one launch, one workgroup per sample:
// choose the [MASK] positions to reveal, write their tokens, pad behind the first EOS, write the conditioning back.
//
//   k            min(sched[b], number of [MASK] positions of the row); k <= 0 reveals nothing
//   confidence   conf_l = logp_l + (r_temp g_l) t_b, three rounded fp32 operations in this order (`_maskgit_update`, model_eval.py:3046-3114); thr = the k-th
//                largest over the [MASK] positions; EVERY [MASK] position with conf >= thr takes its token (ties at the threshold are all revealed)
//   lottery      exactly the k [MASK] positions with the largest values, ordered by (value descending, position ascending) (`_first_hitting_update`,
//                model_eval.py:3005-3043, with the order of equal values defined)
//   EOS rule     first = the smallest l with x_new[l] == eos_id; every l > first with modality 0 whose token is neither pad nor [MASK] becomes pad
//                (model_eval.py:2390-2394)
//   write-back   x_new = x0 where x0_unmask (model_eval.py:2399)
//
// The row lives in registers: thread t of NT owns the positions i NT + t, i < VPT (reveal_plan.h).  The step's compacted results (rows, tok, logp) are
// matched to positions through LDS: the sample's segment of `rows` is found by binary search within [0, n), every entry is range-checked against the sample's
// positions and leaves its index at slot[position]; a [MASK] position nobody wrote has log p = -inf and keeps [MASK].  Selection is exact and needs no sort:
// the k-th largest value is found bit by bit on the order-preserving 32-bit key of the fp32 value (32 block counts), the lottery's cut among equal values by
// bisection on the position.  Counts are ballots summed over the waves in a fixed order: two launches are bit-identical.
#include "common.h"
#include "reveal_plan.h"
#include "../../include/unidisc_hip.h"

namespace {
using namespace udm;

struct RevArgs {
  const int64_t* x;
  int64_t* x_out;
  const int64_t* rows;
  const int64_t* tok;
  const float* logp;
  const int64_t* sched;        // nullable: nothing is revealed
  const float* t;
  const float* noise;          // nullable: Philox
  float* out_noise;            // nullable
  const int64_t* modality;
  const int64_t* x0;
  const uint8_t* unmask;
  long ldx, ldo, ldn, ldon, ldm, ld0, n;
  uint64_t seed;
  float r_temp;
  int L, lottery;
  int64_t mask_id, eos_id, pad_id;
};

// monotone map of fp32 onto uint32: a < b as floats <=> key(a) < key(b) as integers (-0 is folded onto +0 by the callers)
__device__ __forceinline__ uint32_t fkey(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// u = ((r >> 8) + 0.5) 2^-24 in (0, 1), Gumbel = -log(-log u).  x + 0.5 has 25 bits for x >= 2^23 and fp32 rounds it to an integer (u = 1, a Gumbel of +inf,
// at the top of the grid), so the upper half is held as 1 - u = ((2^24 - 1 - x) + 0.5) 2^-24, which is exact, and -log(u) = -log1p(-(1 - u))
__device__ __forceinline__ float gumbel_of(uint32_t r) {
  const uint32_t x = r >> 8;
  const float e = x < (1u << 23) ? -__logf(((float)x + 0.5f) * (1.0f / 16777216.0f)) : -log1pf(-(((float)(0xFFFFFFu - x) + 0.5f) * (1.0f / 16777216.0f)));
  return -__logf(e);
}
// the lottery value: that grid point rounded to fp32, kept below 1 (the top of the grid would round to 1)
__device__ __forceinline__ float uniform_of(uint32_t r) { return fminf(((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f), 0.99999994f); }

// sum of a wave-uniform value over the waves of the block: one barrier per call on a double-buffered slot (a slot is rewritten two calls later, behind the
// barrier of the call in between)
template <int NW>
__device__ __forceinline__ int block_sum(int v, int* red, int& rd) {
  if (NW == 1) return v;
  int* s = red + (rd & 1) * 16;
  ++rd;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += s[w];
  return t;
}
template <int NW>
__device__ __forceinline__ int block_min(int v, int* red, int& rd) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  if (NW == 1) return v;
  int* s = red + (rd & 1) * 16;
  ++rd;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = min(t, s[w]);
  return t;
}
// logp + (r_temp g) t with three roundings.  hipcc contracts a * b + c into a fused multiply-add by default (-ffp-contract=fast), also through __fmul_rn /
// __fadd_rn, which are plain operators in HIP: the pragma takes the contract flag off these three operations, wherever the function is inlined.
__device__ __forceinline__ float confidence(float lp, float r_temp, float g, float t) {
#pragma clang fp contract(off)
  const float rg = r_temp * g;
  const float rgt = rg * t;
  return lp + rgt;
}
__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// the first index in [0, n) whose entry is >= v (n when none is): every probe stays inside [0, n)
__device__ __forceinline__ long lower_bound(const int64_t* rows, long n, int64_t v) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (rows[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int NT, int VPT>
__global__ __launch_bounds__(NT) void reveal_rows_kernel(RevArgs a) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  constexpr int NW = NT / 64;
  int* slot = lds;               // [NT VPT]: index into rows / tok / logp of the entry that names the position, -1: none
  int* red = lds + NT * VPT;     // [2][16]
  const long b = blockIdx.x;
  const int tid = threadIdx.x, L = a.L;
  int rd = 0;

  int64_t xv[VPT];
  bool m[VPT];
  int c = 0;
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int l = i * NT + tid;
    xv[i] = l < L ? a.x[b * a.ldx + l] : 0;
    m[i] = l < L && xv[i] == a.mask_id;
    c += wave_count(m[i]);
  }
  const int n_mask = block_sum<NW>(c, red, rd);
  const int64_t want = a.sched ? a.sched[b] : 0;
  const int k = want < (int64_t)n_mask ? (want > 0 ? (int)want : 0) : n_mask;

  float nz[VPT];
  if (k > 0 || a.out_noise) {
    const uint64_t base = (uint64_t)b * (uint64_t)((L + 3) / 4);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int l = i * NT + tid;
      nz[i] = 0.f;
      if (l >= L) continue;
      if (a.noise) {
        nz[i] = a.noise[b * a.ldn + l];
      } else {
        const uint4 r = philox4x32(a.seed, base + (uint64_t)(l >> 2));
        const uint32_t w = (l & 3) == 0 ? r.x : ((l & 3) == 1 ? r.y : ((l & 3) == 2 ? r.z : r.w));
        nz[i] = a.lottery ? uniform_of(w) : gumbel_of(w);
      }
      if (a.out_noise) a.out_noise[b * a.ldon + l] = nz[i];
    }
  }

  bool rev[VPT];
  int64_t tk[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) { rev[i] = false; tk[i] = xv[i]; }
  if (k > 0) {   // (k is the same in every thread of the block: the barriers below are reached by all or by none)
#pragma unroll
    for (int i = 0; i < VPT; ++i) slot[i * NT + tid] = -1;
    __syncthreads();
    const int64_t p0 = (int64_t)b * L;
    const long s0 = lower_bound(a.rows, a.n, p0), s1 = lower_bound(a.rows, a.n, p0 + L);
    for (long j = s0 + tid; j < s1; j += NT) {
      const int64_t r = a.rows[j] - p0;
      if (r >= 0 && r < L) slot[r] = (int)j;    // (rows out of order: the segment may hold entries of other samples)
    }
    __syncthreads();
    const float tb = a.lottery ? 0.f : a.t[b];
    uint32_t key[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      key[i] = 0;
      if (!m[i]) continue;
      const int s = slot[i * NT + tid];
      if (s >= 0) tk[i] = a.tok[s];
      float v;
      if (a.lottery) {
        v = nz[i];
      } else {
        const float lp = s >= 0 ? a.logp[s] : -INFINITY;
        v = confidence(lp, a.r_temp, nz[i], tb);
      }
      key[i] = fkey(__fadd_rn(v, 0.0f));   // -0 + 0 = +0
    }
    // the k-th largest key among the [MASK] positions: the largest T with #{key >= T} >= k, one bit per round
    uint32_t T = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = T | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < VPT; ++i) cnt += wave_count(m[i] && key[i] >= cand);
      if (block_sum<NW>(cnt, red, rd) >= k) T = cand;
    }
    if (!a.lottery) {
#pragma unroll
      for (int i = 0; i < VPT; ++i) rev[i] = m[i] && key[i] >= T;
    } else {
      int n_gt = 0, n_eq = 0;
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        n_gt += wave_count(m[i] && key[i] > T);
        n_eq += wave_count(m[i] && key[i] == T);
      }
      n_gt = block_sum<NW>(n_gt, red, rd);
      n_eq = block_sum<NW>(n_eq, red, rd);
      const int need = k - n_gt;   // >= 1 of the n_eq values equal to the k-th: the first `need` by position
      int cut = L;
      if (need < n_eq) {           // the smallest P with #{equal values at l < P} >= need
        int plo = 1, phi = L;
        while (plo < phi) {
          const int mid = plo + ((phi - plo) >> 1);
          int cnt = 0;
#pragma unroll
          for (int i = 0; i < VPT; ++i) cnt += wave_count(m[i] && key[i] == T && i * NT + tid < mid);
          if (block_sum<NW>(cnt, red, rd) >= need) phi = mid; else plo = mid + 1;
        }
        cut = plo;
      }
#pragma unroll
      for (int i = 0; i < VPT; ++i) rev[i] = m[i] && (key[i] > T || (key[i] == T && i * NT + tid < cut));
    }
  }

  int64_t xn[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) xn[i] = rev[i] ? tk[i] : xv[i];
  if (a.eos_id >= 0) {
    int first = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int l = i * NT + tid;
      if (l < L && xn[i] == a.eos_id) first = min(first, l);
    }
    first = block_min<NW>(first, red, rd);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int l = i * NT + tid;
      if (l < L && l > first && xn[i] != a.pad_id && xn[i] != a.mask_id && a.modality[b * a.ldm + l] == 0) xn[i] = a.pad_id;
    }
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int l = i * NT + tid;
    if (l >= L) continue;
    if (a.unmask && a.unmask[b * a.ld0 + l]) xn[i] = a.x0[b * a.ld0 + l];
    a.x_out[b * a.ldo + l] = xn[i];
  }
}

template <int NT, int VPT>
void launch(const RevArgs& a, unsigned B, const RevealPlan& p, hipStream_t stream) {
  hipLaunchKernelGGL((reveal_rows_kernel<NT, VPT>), dim3(B), dim3(NT), p.lds_bytes, stream, a);
}

}  // namespace

extern "C" int udm_reveal_rows(const int64_t* x, int64_t ldx, int64_t* x_out, int64_t ldo, const int64_t* rows, const int64_t* tok, const float* logp, int64_t n,
                               const int64_t* sched, const float* t, const float* noise, int64_t ldn, float* out_noise, int64_t ldon, uint64_t seed, float r_temp,
                               int lottery, int64_t eos_id, int64_t pad_id, const int64_t* modality, int64_t ldm, const int64_t* x0, const void* x0_unmask,
                               int64_t ld0, int64_t B, int64_t L, int64_t mask_id, hipStream_t stream) {
  if (B == 0) return 0;
  UDM_CHECK_ARG(x && x_out, "udm_reveal_rows: null pointer");
  UDM_CHECK_ARG(x != x_out, "udm_reveal_rows: x_out is out of place, it must not be x");
  UDM_CHECK_ARG(B > 0 && B < (1L << 20) && L >= 1, "udm_reveal_rows: bad shape B=%ld L=%ld", (long)B, (long)L);
  const RevealPlan p = reveal_plan(L);
  UDM_CHECK_ARG(p.ok, "udm_reveal_rows: L=%ld > %d (the row is held in registers)", (long)L, REVEAL_L_MAX);
  UDM_CHECK_ARG(ldx >= L && ldo >= L, "udm_reveal_rows: row stride of x / x_out smaller than L");
  UDM_CHECK_ARG(n >= 0 && n < (1L << 31), "udm_reveal_rows: bad row count n=%ld", (long)n);
  UDM_CHECK_ARG(n == 0 || (rows && tok), "udm_reveal_rows: n > 0 needs rows and tok");
  UDM_CHECK_ARG(lottery == 0 || lottery == 1, "udm_reveal_rows: lottery must be 0 or 1");
  UDM_CHECK_ARG(lottery || !sched || t, "udm_reveal_rows: the confidence mode needs t");
  UDM_CHECK_ARG(lottery || n == 0 || logp, "udm_reveal_rows: the confidence mode needs logp");
  UDM_CHECK_ARG(!noise || ldn >= L, "udm_reveal_rows: noise row stride smaller than L");
  UDM_CHECK_ARG(!out_noise || ldon >= L, "udm_reveal_rows: out_noise row stride smaller than L");
  UDM_CHECK_ARG(eos_id < 0 || (modality && ldm >= L && pad_id >= 0), "udm_reveal_rows: the EOS rule needs pad_id >= 0 and the modality map");
  UDM_CHECK_ARG((x0 == nullptr) == (x0_unmask == nullptr) && (!x0 || ld0 >= L), "udm_reveal_rows: the write-back needs x0 and x0_unmask with a row stride >= L");
  RevArgs a{};
  a.x = x; a.x_out = x_out; a.rows = rows; a.tok = tok; a.logp = logp; a.sched = sched; a.t = t; a.noise = noise; a.out_noise = out_noise;
  a.modality = modality; a.x0 = x0; a.unmask = (const uint8_t*)x0_unmask;
  a.ldx = ldx; a.ldo = ldo; a.ldn = ldn; a.ldon = ldon; a.ldm = ldm; a.ld0 = ld0; a.n = n;
  a.seed = seed; a.r_temp = r_temp; a.L = (int)L; a.lottery = lottery; a.mask_id = mask_id; a.eos_id = eos_id; a.pad_id = pad_id;
  const unsigned nb = (unsigned)B;
  if (p.threads == 64) launch<64, 1>(a, nb, p, stream);
  else if (p.threads == 256 && p.vpt == 1) launch<256, 1>(a, nb, p, stream);
  else if (p.threads == 256) launch<256, 4>(a, nb, p, stream);
  else if (p.vpt == 2) launch<1024, 2>(a, nb, p, stream);
  else if (p.vpt == 4) launch<1024, 4>(a, nb, p, stream);
  else launch<1024, 8>(a, nb, p, stream);
  UDM_CHECK_LAUNCH("udm_reveal_rows");
  return 0;
}
