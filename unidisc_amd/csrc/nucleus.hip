// Top-p (nucleus) token choice from materialised bf16 logits, one workgroup per row, without a sort.
//
//   valid ids   id < V, id != mask_id and, with restrict_modality, the row's modality only (text ids are < Vt)
//   z           logits, or (1 + w) logits - w logits_uncond with every operation rounded to fp32 (`cfg`, model_eval.py:2630-2640)
//   e_i         exp2((z_i - max z) inv_temperature log2(e)) = p_i Z,  Z = sum e
//   order       descending e, ascending id among equal values (the stable order; torch.sort leaves ties unspecified)
//   kept set    the longest prefix of that order whose mass is <= budget Z; the first id is always kept
//   token       argmax over the kept ids of e_i / (1e-10 - log(u_i + 1e-10)), first index on ties (`_sample_categorical`, model_utils.py:95-97)
//
// `nucleus_sampling_batch` (model_eval.py:2642-2685: p / T against top_p) is inv_temperature = 1, budget = top_p T; `nucleus_sampling` (:2691-2734) is
// inv_temperature = 1 / T, budget = top_p.  The hosts map; the kernel knows neither rule.
//
// The row is read from global memory once per operand and then lives in registers: 1024 threads x NG groups of 8 ids, thread t owns the ids
// (i 1024 + t) 8 + j.  Selection is bisection, every round one pass over the registers and one block sum:
//   A  on the bit pattern k of e (non-negative floats order as integers): the smallest k with mass{e >= k} <= budget Z, at most 31 rounds
//   B  the ties at the next lower value v = k - 1 (present, or round A would have stopped lower): the c that still fit, acc + c v <= budget Z, are the
//      first c in id order; their last id is found by bisection on the id, at most 17 rounds of an integer count
// Every sum is the same fixed tree (per thread in (i, j) order, xor butterfly per wave, the 16 waves in order): no atomics of any kind, two launches are
// bit-identical, and since rounded addition is monotone the mass is monotone in k, so the bisection is well defined.
#include "common.h"
#include "../../include/unidisc_hip.h"

namespace {
using namespace udm;
constexpr int NT = 1024;                // threads per workgroup
constexpr int NW = NT / 64;             // waves
constexpr int KEY_ONE = 0x3F800000;     // e = 1: the row maximum

struct NucArgs {
  const bf16_t* logits;
  const bf16_t* logits_u;      // nullable
  const float* w;              // per row, or one scalar (w_scalar)
  const int64_t* modality;     // modality[row * ldm + mod_col]
  const float* u;              // u[row * ldu + u_col0 + id], nullable = Philox
  int64_t* out;                // rows entry: token per row (nullable)
  float* out_logp;             // nullable
  int64_t* out_keep;           // nullable
  int64_t* x;                  // AR entry: x[r, pos] write-back (nullable = rows entry)
  const int64_t* x0;
  const uint8_t* unmask;
  int64_t* next_ids;
  long ld, ldm, mod_col, ldu, u_col0, ldx, pos, step;
  uint64_t seed;
  float inv_temperature, budget;
  int R, V, Vt, mask_id, restrict_modality, w_scalar;
  const int64_t* pos_dev;      // the device-position AR entry (AT): pos = mod_col = i + 1, step = i, u_col0 = i V with i = *pos_dev
};

struct Red {
  float f[2][NW];
  int i[2][NW];
};

// block sums over a double-buffered slot: one barrier per call (a slot is rewritten two calls later, behind the barrier of the call in between)
__device__ __forceinline__ float block_sum_f(float v, Red& r, int& rd) {
  v = wave_sum(v);
  float* s = r.f[rd & 1];
  ++rd;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += s[w];
  return t;
}
__device__ __forceinline__ int block_sum_i(int v, Red& r, int& rd) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  int* s = r.i[rd & 1];
  ++rd;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += s[w];
  return t;
}
__device__ __forceinline__ float block_max_f(float v, Red& r, int& rd) {
  v = wave_max(v);
  float* s = r.f[rd & 1];
  ++rd;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = s[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = fmaxf(t, s[w]);
  return t;
}

template <int NG>
__device__ __forceinline__ float mass_ge(const float (&e)[NG][8], int k, Red& r, int& rd) {   // invalid ids hold -1 (a negative key): never >= k
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (__float_as_int(e[i][j]) >= k) ? e[i][j] : 0.f;
  return block_sum_f(s, r, rd);
}

__device__ __forceinline__ float mix(float c, float u, float gw) { return __fsub_rn(__fmul_rn(1.0f + gw, c), __fmul_rn(gw, u)); }

template <int NG, bool GUIDED, bool AT>
__global__ __launch_bounds__(NT) void nucleus_rows_kernel(NucArgs a) {
  __shared__ Red red;
  __shared__ float bs[NW];
  __shared__ int bi[NW];
  if (AT) {   // (block-uniform, before any barrier) a position whose column, modality column or noise columns do not exist: nothing is stored
    const long i = *a.pos_dev;
    if (i < 0 || i + 1 >= a.ldx || (a.restrict_modality && i + 1 >= a.ldm) || (a.u && (i + 1) * (long)a.V > a.ldu)) return;
    a.pos = a.mod_col = i + 1, a.step = i, a.u_col0 = i * (long)a.V;
  }
  const long row = blockIdx.x;
  const int tid = threadIdx.x;
  int rd = 0;
  int lo = 0, hi = a.V;
  if (a.restrict_modality) {
    const bool img = a.modality[row * a.ldm + a.mod_col] == 1;
    if (img) lo = a.Vt; else hi = a.Vt;
  }
  const bf16_t* zc = a.logits + row * a.ld;
  const bf16_t* zu = GUIDED ? a.logits_u + row * a.ld : nullptr;
  const float gw = GUIDED ? (a.w_scalar ? a.w[0] : a.w[row]) : 0.f;

  // ---- the one read of the row: z in registers, -inf on every id that is not valid (whatever those columns hold, NaN included, is dropped here)
  // (all loads are issued first, then unpacked group by group: the scheduler barriers keep the register peak at raw + e instead of interleaving everything)
  uint4 raw[NG], rawu[GUIDED ? NG : 1];
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c = (i * NT + tid) * 8;
    raw[i] = make_uint4(0, 0, 0, 0);
    if (GUIDED) rawu[i] = make_uint4(0, 0, 0, 0);
    if (c < hi && c + 8 > lo) {
      raw[i] = *reinterpret_cast<const uint4*>(zc + c);
      if (GUIDED) rawu[i] = *reinterpret_cast<const uint4*>(zu + c);
    }
  }
  float e[NG][8];
  float zmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c = (i * NT + tid) * 8;
    const uint32_t wd[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(wd[k] << 16); v[2 * k + 1] = __uint_as_float(wd[k] & 0xffff0000u); }
    if (GUIDED) {
      const uint32_t wu[4] = {rawu[i].x, rawu[i].y, rawu[i].z, rawu[i].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = mix(v[2 * k], __uint_as_float(wu[k] << 16), gw);
        v[2 * k + 1] = mix(v[2 * k + 1], __uint_as_float(wu[k] & 0xffff0000u), gw);
      }
    }
    // id = c + j is valid iff rlo <= j < rhi and j != rmask: per-group offsets, so that no per-id register lives on (64 of them would not fit)
    const int rlo = lo - c, rhi = hi - c, rmask = a.mask_id - c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = j >= rlo && j < rhi && j != rmask;   // also false for every id of a group that was not loaded
      e[i][j] = ok ? v[j] : -INFINITY;
      zmax = fmaxf(zmax, e[i][j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  zmax = block_max_f(zmax, red, rd);

  // ---- e = exp2((z - max) scale), -1 on invalid ids; Z1 = the un-tempered sum (log p_1 of the token is reported against it)
  const float LOG2E = 1.4426950408889634f;
  const float scale = a.inv_temperature * LOG2E;
  const bool tempered = a.inv_temperature != 1.0f;
  // (d = z - max in place first: with z and d both alive the compiler holds two copies of the row)
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) e[i][j] -= zmax;   // -inf on invalid ids
  float s1 = 0.f;
  if (tempered) {
#pragma unroll
    for (int i = 0; i < NG; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) s1 += __builtin_amdgcn_exp2f(e[i][j] * LOG2E);   // exp2(-inf) = 0
  }
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = e[i][j];
      e[i][j] = d != -INFINITY ? __builtin_amdgcn_exp2f(d * scale) : -1.0f;
    }
  const float Z = mass_ge<NG>(e, 0, red, rd);
  const float Z1 = tempered ? block_sum_f(s1, red, rd) : Z;
  const float Bu = a.budget * Z;

  // ---- A: the smallest key k with mass{e >= k} <= Bu (k = KEY_ONE + 1 selects nothing)
  int klo = 0, khi = KEY_ONE + 1;
  float acc = 0.f;
  while (klo < khi) {
    const int mid = klo + ((khi - klo) >> 1);
    const float m = mass_ge<NG>(e, mid, red, rd);
    if (m <= Bu) { khi = mid; acc = m; } else klo = mid + 1;
  }
  const int kstar = klo;
  const int vkey = kstar - 1;   // kstar = 0: everything is kept and -1 is nobody's key
  int n_hi = 0, c_v = 0;
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = __float_as_int(e[i][j]);
      n_hi += (k >= kstar) ? 1 : 0;
      c_v += (k == vkey) ? 1 : 0;
    }
  n_hi = block_sum_i(n_hi, red, rd);
  c_v = block_sum_i(c_v, red, rd);

  // ---- B: how many of the c_v ties at v fit, and the id below which they lie
  int c = 0;
  if (c_v > 0) {
    const float v = __int_as_float(vkey);
    if (v > 0.f) {
      const float cf = floorf((Bu - acc) / v);
      c = cf >= (float)c_v ? c_v : (cf > 0.f ? (int)cf : 0);
      for (int it = 0; it < 2; ++it)
        if (c > 0 && __fmaf_rn((float)c, v, acc) > Bu) --c;
      for (int it = 0; it < 2; ++it)
        if (c < c_v && __fmaf_rn((float)(c + 1), v, acc) <= Bu) ++c;
    } else {
      c = c_v;
    }
    if (n_hi + c == 0) c = 1;   // the top id always stays
  }
  int tcut = 0;
  if (c >= c_v) {
    tcut = 0x7fffffff;
  } else if (c > 0) {
    int tlo = 1, thi = a.V;   // the smallest T with #{ties with id < T} >= c
    while (tlo < thi) {
      const int mid = tlo + ((thi - tlo) >> 1);
      int n = 0;
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const int rel = mid - (i * NT + tid) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) n += (__float_as_int(e[i][j]) == vkey && j < rel) ? 1 : 0;
      }
      n = block_sum_i(n, red, rd);
      if (n >= c) thi = mid; else tlo = mid + 1;
    }
    tcut = tlo;
  }

  // ---- the race over the kept ids
  const uint64_t pkey = a.x ? a.seed ^ ((uint64_t)(a.step + 1) * 0x9E3779B97F4A7C15ull) : a.seed;
  const uint64_t pbase = a.x ? ((uint64_t)row << 40) : (uint64_t)row * (uint64_t)((a.V + 3) / 4);
  const float* ur = a.u ? a.u + row * a.ldu + a.u_col0 : nullptr;
  float best = -1.f;
  int besti = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c0 = (i * NT + tid) * 8;
    const int rcut = tcut > c0 ? tcut - c0 : 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bool kept[4];
      bool any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = __float_as_int(e[i][4 * q + j]);
        kept[j] = k >= kstar || (k == vkey && 4 * q + j < rcut);
        any = any || kept[j];
      }
      if (!any) continue;
      uint4 r = make_uint4(0, 0, 0, 0);
      if (!ur) r = philox4x32(pkey, pbase + (uint64_t)((c0 >> 2) + q));
      const uint32_t rw[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!kept[j]) continue;
        const float uu = ur ? ur[c0 + 4 * q + j] : (float)(rw[j] >> 8) * (1.0f / 16777216.0f);
        const float score = e[i][4 * q + j] / (1e-10f - logf(uu + 1e-10f));
        if (score > best) { best = score; besti = c0 + 4 * q + j; }   // ids increase per thread: the first maximum is kept
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float b2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(besti, o, 64);
    if (b2 > best || (b2 == best && i2 < besti)) { best = b2; besti = i2; }
  }
  if ((tid & 63) == 0) { bs[tid >> 6] = best; bi[tid >> 6] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w)
      if (bs[w] > best || (bs[w] == best && bi[w] < besti)) { best = bs[w]; besti = bi[w]; }
    const bool found = besti >= lo && besti < hi;   // (no admissible id: cannot happen without NaN among the valid logits)
    const int tok = found ? besti : lo;
    if (a.out) a.out[row] = tok;
    if (a.out_keep) a.out_keep[row] = n_hi + c;
    if (a.out_logp) {
      const float zt = GUIDED ? mix(bf2f(zc[tok]), bf2f(zu[tok]), gw) : bf2f(zc[tok]);
      a.out_logp[row] = found ? (zt - zmax) - logf(Z1) : -INFINITY;
    }
    if (a.x) {   // the write-back of udm_ar_sample_rows
      const long at = row * a.ldx + a.pos;
      const bool keep = a.unmask && a.unmask[at];
      const int64_t val = keep ? a.x0[at] : (int64_t)tok;
      a.x[at] = val;
      if (a.next_ids) {
        a.next_ids[row] = val;
        if (GUIDED) a.next_ids[a.R + row] = keep ? a.mask_id : val;
      }
    }
  }
}

template <bool GUIDED, bool AT = false>
void launch_ng(const NucArgs& a, unsigned rows, hipStream_t stream) {
  const int need = ((a.V + 7) / 8 + NT - 1) / NT;   // groups of 8 ids per thread
  if (need <= 1) hipLaunchKernelGGL((nucleus_rows_kernel<1, GUIDED, AT>), dim3(rows), dim3(NT), 0, stream, a);
  else if (need <= 2) hipLaunchKernelGGL((nucleus_rows_kernel<2, GUIDED, AT>), dim3(rows), dim3(NT), 0, stream, a);
  else if (need <= 4) hipLaunchKernelGGL((nucleus_rows_kernel<4, GUIDED, AT>), dim3(rows), dim3(NT), 0, stream, a);
  else if (need <= 6) hipLaunchKernelGGL((nucleus_rows_kernel<6, GUIDED, AT>), dim3(rows), dim3(NT), 0, stream, a);
  else hipLaunchKernelGGL((nucleus_rows_kernel<8, GUIDED, AT>), dim3(rows), dim3(NT), 0, stream, a);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int64_t V_MAX = 65536;   // 1024 threads x 8 groups x 8 ids in registers

}  // namespace

extern "C" int udm_nucleus_sample_rows(const void* logits, const void* logits_uncond, const float* w, int64_t ld, const int64_t* modality, const float* u,
                                       int64_t ldu, uint64_t seed, float inv_temperature, float budget, int64_t* out, float* out_logp, int64_t* out_keep,
                                       int64_t M, int64_t V, int64_t Vt, int64_t mask_id, int restrict_modality, hipStream_t stream) {
  if (M == 0) return 0;
  UDM_CHECK_ARG(logits && out && out_logp, "udm_nucleus_sample_rows: null pointer");
  UDM_CHECK_ARG(M > 0 && M < (1L << 31) && V >= 1 && ld >= V && ld % 8 == 0 && Vt >= 0 && Vt <= V, "udm_nucleus_sample_rows: bad shape M=%ld V=%ld ld=%ld Vt=%ld",
                (long)M, (long)V, (long)ld, (long)Vt);
  UDM_CHECK_ARG(V <= V_MAX, "udm_nucleus_sample_rows: V=%ld > %ld (the row is held in registers)", (long)V, (long)V_MAX);
  UDM_CHECK_ARG(inv_temperature > 0.f && budget > 0.f, "udm_nucleus_sample_rows: inv_temperature and budget must be positive");
  UDM_CHECK_ARG(!u || ldu >= V, "udm_nucleus_sample_rows: noise row stride too small");
  UDM_CHECK_ARG(!restrict_modality || modality, "udm_nucleus_sample_rows: restrict_modality needs the per-row modality");
  UDM_CHECK_ARG((logits_uncond == nullptr) == (w == nullptr), "udm_nucleus_sample_rows: guidance needs both the unconditional logits and the per-row weights");
  UDM_CHECK_ARG(al16(logits) && al16(logits_uncond), "udm_nucleus_sample_rows: logits must be 16-byte aligned");
  NucArgs a{};
  a.logits = (const bf16_t*)logits; a.logits_u = (const bf16_t*)logits_uncond; a.w = w; a.modality = modality; a.u = u;
  a.out = out; a.out_logp = out_logp; a.out_keep = out_keep;
  a.ld = ld; a.ldm = 1; a.mod_col = 0; a.ldu = ldu; a.u_col0 = 0;
  a.seed = seed; a.inv_temperature = inv_temperature; a.budget = budget;
  a.R = (int)M; a.V = (int)V; a.Vt = (int)Vt; a.mask_id = (int)mask_id; a.restrict_modality = restrict_modality; a.w_scalar = 0;
  if (logits_uncond) launch_ng<true>(a, (unsigned)M, stream); else launch_ng<false>(a, (unsigned)M, stream);
  UDM_CHECK_LAUNCH("udm_nucleus_sample_rows");
  return 0;
}

extern "C" int udm_ar_nucleus_rows(const void* logits, const void* logits_uncond, const float* w, int64_t ld, const int64_t* modality, int64_t ldm, const float* u,
                                   int64_t ldu, int64_t u_col0, uint64_t seed, int64_t step, float inv_temperature, float budget, int64_t* x, int64_t ldx,
                                   const int64_t* x0, const void* x0_unmask, int64_t pos, int64_t* next_ids, int64_t R, int64_t V, int64_t Vt, int64_t mask_id,
                                   int restrict_modality, hipStream_t stream) {
  UDM_CHECK_ARG(logits && x, "udm_ar_nucleus_rows: null pointer");
  UDM_CHECK_ARG(R >= 1 && R < (1L << 20) && V >= 1 && ld >= V && ld % 8 == 0 && pos >= 0 && pos < ldx, "udm_ar_nucleus_rows: bad shape R=%ld V=%ld ld=%ld pos=%ld",
                (long)R, (long)V, (long)ld, (long)pos);
  UDM_CHECK_ARG(V <= V_MAX, "udm_ar_nucleus_rows: V=%ld > %ld (the row is held in registers)", (long)V, (long)V_MAX);
  UDM_CHECK_ARG(inv_temperature > 0.f && budget > 0.f, "udm_ar_nucleus_rows: inv_temperature and budget must be positive");
  UDM_CHECK_ARG(!logits_uncond || w, "udm_ar_nucleus_rows: guidance needs the weight");
  UDM_CHECK_ARG(!restrict_modality || (modality && ldm > pos && Vt > 0 && Vt < V), "udm_ar_nucleus_rows: the restriction needs the modality map and 0 < Vt < V");
  UDM_CHECK_ARG(!x0_unmask || x0, "udm_ar_nucleus_rows: x0_unmask needs x0");
  UDM_CHECK_ARG(!u || (ldu >= u_col0 + V && u_col0 >= 0), "udm_ar_nucleus_rows: bad noise layout");
  UDM_CHECK_ARG(al16(logits) && al16(logits_uncond), "udm_ar_nucleus_rows: logits must be 16-byte aligned");
  NucArgs a{};
  a.logits = (const bf16_t*)logits; a.logits_u = (const bf16_t*)logits_uncond; a.w = w; a.modality = modality; a.u = u;
  a.x = x; a.x0 = x0; a.unmask = (const uint8_t*)x0_unmask; a.next_ids = next_ids;
  a.ld = ld; a.ldm = ldm; a.mod_col = pos; a.ldu = ldu; a.u_col0 = u_col0; a.ldx = ldx; a.pos = pos; a.step = step;
  a.seed = seed; a.inv_temperature = inv_temperature; a.budget = budget;
  a.R = (int)R; a.V = (int)V; a.Vt = (int)Vt; a.mask_id = (int)mask_id; a.restrict_modality = restrict_modality; a.w_scalar = 1;
  if (logits_uncond) launch_ng<true>(a, (unsigned)R, stream); else launch_ng<false>(a, (unsigned)R, stream);
  UDM_CHECK_LAUNCH("udm_ar_nucleus_rows");
  return 0;
}

extern "C" int udm_ar_nucleus_rows_at(const void* logits, const void* logits_uncond, const float* w, int64_t ld, const int64_t* modality, int64_t ldm,
                                      const float* u, int64_t ldu, uint64_t seed, float inv_temperature, float budget, int64_t* x, int64_t ldx,
                                      const int64_t* x0, const void* x0_unmask, const int64_t* pos_dev, int64_t* next_ids, int64_t R, int64_t V, int64_t Vt,
                                      int64_t mask_id, int restrict_modality, hipStream_t stream) {
  UDM_CHECK_ARG(logits && x && pos_dev && ((uintptr_t)pos_dev & 7) == 0, "udm_ar_nucleus_rows_at: null pointer (the position must be an aligned device int64)");
  UDM_CHECK_ARG(R >= 1 && R < (1L << 20) && V >= 1 && ld >= V && ld % 8 == 0 && ldx >= 1, "udm_ar_nucleus_rows_at: bad shape R=%ld V=%ld ld=%ld ldx=%ld", (long)R,
                (long)V, (long)ld, (long)ldx);
  UDM_CHECK_ARG(V <= V_MAX, "udm_ar_nucleus_rows_at: V=%ld > %ld (the row is held in registers)", (long)V, (long)V_MAX);
  UDM_CHECK_ARG(inv_temperature > 0.f && budget > 0.f, "udm_ar_nucleus_rows_at: inv_temperature and budget must be positive");
  UDM_CHECK_ARG(!logits_uncond || w, "udm_ar_nucleus_rows_at: guidance needs the weight");
  UDM_CHECK_ARG(!restrict_modality || (modality && ldm >= 1 && Vt > 0 && Vt < V), "udm_ar_nucleus_rows_at: the restriction needs the modality map and 0 < Vt < V");
  UDM_CHECK_ARG(!x0_unmask || x0, "udm_ar_nucleus_rows_at: x0_unmask needs x0");
  UDM_CHECK_ARG(!u || ldu >= V, "udm_ar_nucleus_rows_at: bad noise layout");
  UDM_CHECK_ARG(al16(logits) && al16(logits_uncond), "udm_ar_nucleus_rows_at: logits must be 16-byte aligned");
  NucArgs a{};
  a.logits = (const bf16_t*)logits; a.logits_u = (const bf16_t*)logits_uncond; a.w = w; a.modality = modality; a.u = u;
  a.x = x; a.x0 = x0; a.unmask = (const uint8_t*)x0_unmask; a.next_ids = next_ids;
  a.ld = ld; a.ldm = ldm; a.ldu = ldu; a.ldx = ldx; a.pos_dev = pos_dev;
  a.seed = seed; a.inv_temperature = inv_temperature; a.budget = budget;
  a.R = (int)R; a.V = (int)V; a.Vt = (int)Vt; a.mask_id = (int)mask_id; a.restrict_modality = restrict_modality; a.w_scalar = 1;
  if (logits_uncond) launch_ng<true, true>(a, (unsigned)R, stream); else launch_ng<false, true>(a, (unsigned)R, stream);
  UDM_CHECK_LAUNCH("udm_ar_nucleus_rows_at");
  return 0;
}
