// KV-cached next-token decoding of the AR baseline (`_ar_sampler`, model_eval.py:2736-2822, cache models/dit.py:588-607, 776-780, 1462-1473): the three
// kernels a decode step needs that the training path has no form for.
//
//   udm_gemm_skinny_bf16   out[M, N] = A[M, K] W[N, K]^T for M <= 128 (the B rows of a decode step): weight streaming.  Every weight byte is read from HBM
//                          by exactly one workgroup.  A wave owns 32 output columns over a K range and loads its operands straight to VGPRs (16 B per lane,
//                          four 32-deep k-steps in flight) for 16x16x32 MFMAs; the four waves of a workgroup split the workgroup's K range and sum through
//                          LDS.  Where the column tiles alone leave CUs idle (N = d out-projection, K = 4 d down-projection) K is also split over
//                          workgroups: fp32 partial slabs in `ws` and a second launch that sums them and applies the epilogue (the split: skinny_plan.h).
//                          M <= 64 is one group of up to four 16-row tiles (skinny_gemm_kernel); 65 <= M <= 128 is two such groups, rows [0, 64) and
//                          [64, M), in one workgroup on the same weight fragments (skinny_gemm2_kernel), each group bit-identical to a call on its rows.
//   udm_attention_decode   one query row per (b, h) against the per-layer cache, all rows at the same position p (flash-decoding): the keys are split
//                          over workgroups so that B H x splits covers the chip; each split keeps fp32 (m, l, acc) and a second launch combines them.  The
//                          new key / value row is read from its producer for key p and written to cache slot p by the split that owns p - no other
//                          workgroup of the launch reads slot p, so the append needs no ordering.
//   udm_ar_sample_rows     the token choice: argmax(z + Gumbel) over one row per block, z = logits or (1 + w) l_c - w l_u in fp32 with [MASK] and (by next
//                          modality) the other modality's ids excluded, and the chosen id written straight into x[b, pos] (x0 write-back applied) and into
//                          the next step's input ids - the token loop never reads the device.
//
// The device-position forms (a captured graph replays one step for every token; its launches cannot take the position as an argument):
//   udm_attention_decode_at   the same kernel bodies (template parameter AT) on a fixed grid (B H, S bound): each workgroup reads p from device memory,
//                          derives S and chunk with decode_plan.h - the rule the host form evaluates - and leaves if it has no split; the combine launch
//                          is always made and leaves when S = 1.  Same arithmetic, same order: bit-identical to udm_attention_decode(p).
//   udm_ar_sample_rows_at     pos = i + 1, step = i, g_col0 = i V from i = *pos_dev, read in the kernel
//   udm_decode_stage          row p of the modality columns and of the rotary tables into fixed one-row buffers (the embedding and qk-norm + rope kernels
//                          then run unchanged on those); udm_counter_add: position + 1, the last launch of the step
// A position outside its range makes every workgroup return before its first access.  All of these are plain loads and stores.
#include "common.h"
#include "decode_plan.h"
#include "skinny_plan.h"
#include "../../include/unidisc_hip.h"

namespace {

using udm::bf2f;
using udm::f2bf;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;   // 16 bytes as a native vector (what __builtin_nontemporal_load takes)
__device__ __forceinline__ bf16x8_t as_frag(u32x4_t v) { return __builtin_bit_cast(bf16x8_t, v); }

// ------------------------------------------------------------------------------------------------ skinny GEMM
struct SkArgs {
  const bf16_t* A;
  const bf16_t* W;
  void* C;
  float* ws;
  const float* bias;
  long lda, ldw, ldc;
  int M, N, K, kslice, S, out_f32, epi;
};

constexpr int SK_U = 4;          // k-steps of 32 in flight per wave
constexpr int SK_NB = 2;         // 16-column MFMA tiles per wave (32 columns)

__device__ __forceinline__ float sk_epilogue(float v, int n, const SkArgs& a) {
  if (a.epi == UDM_EPI_BIAS || a.epi == UDM_EPI_BIAS_GELU) v += a.bias[n];
  if (a.epi == UDM_EPI_BIAS_GELU) v = udm::gelu_tanh(bf2f(f2bf(v)));   // u = bf16(A W^T + bias), C = gelu(u): the training epilogue's roundings
  return v;
}

__device__ __forceinline__ void sk_store(const SkArgs& a, int m, int n, float v) {
  if (a.out_f32) ((float*)a.C)[(long)m * a.ldc + n] = v;
  else ((bf16_t*)a.C)[(long)m * a.ldc + n] = f2bf(v);
}

template <int MT>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(SkArgs a) {
  __shared__ float red[4 * MT * SK_NB * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 32;
  const int s = blockIdx.y;
  const int kbeg = s * a.kslice;
  const int kend = min(a.K, kbeg + a.kslice);
  const int kl = 8 * (lane >> 4);
  // operand rows of this lane (rows past M / N are clamped to a valid row: their products land in outputs nobody stores)
  const bf16_t* wrow[SK_NB];
#pragma unroll
  for (int nb = 0; nb < SK_NB; ++nb) wrow[nb] = a.W + (long)min(n0 + nb * 16 + (lane & 15), a.N - 1) * a.ldw + kl;
  const bf16_t* arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) arow[mt] = a.A + (long)min(mt * 16 + (lane & 15), a.M - 1) * a.lda + kl;

  f32x4_t acc[MT][SK_NB];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nb = 0; nb < SK_NB; ++nb) acc[mt][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int k0 = kbeg + wave * 32 * SK_U; k0 < kend; k0 += 4 * 32 * SK_U) {
    u32x4_t wf[SK_U][SK_NB], af[SK_U][MT];
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int k = k0 + 32 * u;
      const bool ok = k < kend;   // (K % 32 == 0: a k-step is whole or absent)
#pragma unroll
      for (int nb = 0; nb < SK_NB; ++nb) wf[u][nb] = ok ? __builtin_nontemporal_load((const u32x4_t*)(wrow[nb] + k)) : u32x4_t{0, 0, 0, 0};
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[u][mt] = ok ? *(const u32x4_t*)(arow[mt] + k) : u32x4_t{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nb = 0; nb < SK_NB; ++nb) acc[mt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af[u][mt]), as_frag(wf[u][nb]), acc[mt][nb], 0, 0, 0);
  }
  // the four waves' K ranges summed through LDS; element e = ((mt * NB + nb) * 4 + r) * 64 + lane
  constexpr int E = MT * SK_NB * 4 * 64;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nb = 0; nb < SK_NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * E + ((mt * SK_NB + nb) * 4 + r) * 64 + lane] = acc[mt][nb][r];
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += 256) {
    const float v = red[e] + red[E + e] + red[2 * E + e] + red[3 * E + e];
    const int ln = e & 63, r = (e >> 6) & 3, t = e >> 8;
    const int nb = t % SK_NB, mt = t / SK_NB;
    const int m = mt * 16 + (ln >> 4) * 4 + r, n = n0 + nb * 16 + (ln & 15);
    if (m >= a.M || n >= a.N) continue;
    if (a.S == 1) sk_store(a, m, n, sk_epilogue(v, n, a));
    else a.ws[((long)s * a.M + m) * a.N + n] = v;
  }
}

// 65 <= M <= 128: two row groups in one workgroup.  Group 0 is the rows [0, 64) (four 16-row tiles), group 1 the rows [64, M) (MT1 = 1..4 tiles).  Grid, wave
// layout and K walk are skinny_gemm_kernel's; per k-group a wave loads its W fragments once (non-temporal) and feeds them to both groups' MFMAs, so every
// weight byte is still read from HBM by one workgroup, once.  The A fragments are loaded per group, into the same registers.  Per output element the order of
// the sum is skinny_gemm_kernel's on that element's group: k-steps ascending in a wave, w0 + w1 + w2 + w3 through LDS, the K slabs ascending in
// skinny_reduce_kernel - rows [0, 64) and [64, M) equal, bit for bit, two launches of skinny_gemm_kernel<4> and <MT1> on those rows with the same K split.
// Budget per lane (planned before coding, MT1 = 4): accumulators of both groups (4 + 4) x 2 x 4 = 64, W fragments SK_U x 2 x 4 = 32, one group's A
// fragments SK_U x 4 x 4 = 64, 10 row pointers 20: 180 of the 256 registers that leave two waves per SIMD; amdgpu_waves_per_eu(2) holds the compiler
// to that.  LDS: the cross-wave sum runs per group over the `red` layout of skinny_gemm_kernel<4>, 4 x 2048 floats = 32 KB, as there.
template <int MT1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void skinny_gemm2_kernel(SkArgs a) {
  constexpr int MT0 = 4;
  __shared__ float red[4 * MT0 * SK_NB * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 32;
  const int s = blockIdx.y;
  const int kbeg = s * a.kslice;
  const int kend = min(a.K, kbeg + a.kslice);
  const int kl = 8 * (lane >> 4);
  // (rows past M / N clamped to a valid row, as in skinny_gemm_kernel; group 1 clamps to M - 1, the last row of its own range)
  const bf16_t* wrow[SK_NB];
#pragma unroll
  for (int nb = 0; nb < SK_NB; ++nb) wrow[nb] = a.W + (long)min(n0 + nb * 16 + (lane & 15), a.N - 1) * a.ldw + kl;
  const bf16_t* arow0[MT0];
#pragma unroll
  for (int mt = 0; mt < MT0; ++mt) arow0[mt] = a.A + (long)(mt * 16 + (lane & 15)) * a.lda + kl;
  const bf16_t* arow1[MT1];
#pragma unroll
  for (int mt = 0; mt < MT1; ++mt) arow1[mt] = a.A + (long)min(64 + mt * 16 + (lane & 15), a.M - 1) * a.lda + kl;

  f32x4_t acc0[MT0][SK_NB], acc1[MT1][SK_NB];
#pragma unroll
  for (int nb = 0; nb < SK_NB; ++nb) {
#pragma unroll
    for (int mt = 0; mt < MT0; ++mt) acc0[mt][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT1; ++mt) acc1[mt][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  for (int k0 = kbeg + wave * 32 * SK_U; k0 < kend; k0 += 4 * 32 * SK_U) {
    u32x4_t wf[SK_U][SK_NB], af0[SK_U][MT0], af1[SK_U][MT1];
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int k = k0 + 32 * u;
      const bool ok = k < kend;
#pragma unroll
      for (int nb = 0; nb < SK_NB; ++nb) wf[u][nb] = ok ? __builtin_nontemporal_load((const u32x4_t*)(wrow[nb] + k)) : u32x4_t{0, 0, 0, 0};
#pragma unroll
      for (int mt = 0; mt < MT0; ++mt) af0[u][mt] = ok ? *(const u32x4_t*)(arow0[mt] + k) : u32x4_t{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u)
#pragma unroll
      for (int mt = 0; mt < MT0; ++mt)
#pragma unroll
        for (int nb = 0; nb < SK_NB; ++nb) acc0[mt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af0[u][mt]), as_frag(wf[u][nb]), acc0[mt][nb], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const bool ok = k0 + 32 * u < kend;
#pragma unroll
      for (int mt = 0; mt < MT1; ++mt) af1[u][mt] = ok ? *(const u32x4_t*)(arow1[mt] + k0 + 32 * u) : u32x4_t{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u)
#pragma unroll
      for (int mt = 0; mt < MT1; ++mt)
#pragma unroll
        for (int nb = 0; nb < SK_NB; ++nb) acc1[mt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(af1[u][mt]), as_frag(wf[u][nb]), acc1[mt][nb], 0, 0, 0);
  }
  // the cross-wave sum of skinny_gemm_kernel, once per group: element e = ((mt * NB + nb) * 4 + r) * 64 + lane, row = the group's first row + ...
  constexpr int E0 = MT0 * SK_NB * 4 * 64, E1 = MT1 * SK_NB * 4 * 64;
#pragma unroll
  for (int mt = 0; mt < MT0; ++mt)
#pragma unroll
    for (int nb = 0; nb < SK_NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * E0 + ((mt * SK_NB + nb) * 4 + r) * 64 + lane] = acc0[mt][nb][r];
  __syncthreads();
  for (int e = threadIdx.x; e < E0; e += 256) {
    const float v = red[e] + red[E0 + e] + red[2 * E0 + e] + red[3 * E0 + e];
    const int ln = e & 63, r = (e >> 6) & 3, t = e >> 8;
    const int nb = t % SK_NB, mt = t / SK_NB;
    const int m = mt * 16 + (ln >> 4) * 4 + r, n = n0 + nb * 16 + (ln & 15);
    if (n >= a.N) continue;   // (m < 64 < M)
    if (a.S == 1) sk_store(a, m, n, sk_epilogue(v, n, a));
    else a.ws[((long)s * a.M + m) * a.N + n] = v;
  }
  __syncthreads();   // group 0 has been read out of `red`
#pragma unroll
  for (int mt = 0; mt < MT1; ++mt)
#pragma unroll
    for (int nb = 0; nb < SK_NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * E1 + ((mt * SK_NB + nb) * 4 + r) * 64 + lane] = acc1[mt][nb][r];
  __syncthreads();
  for (int e = threadIdx.x; e < E1; e += 256) {
    const float v = red[e] + red[E1 + e] + red[2 * E1 + e] + red[3 * E1 + e];
    const int ln = e & 63, r = (e >> 6) & 3, t = e >> 8;
    const int nb = t % SK_NB, mt = t / SK_NB;
    const int m = 64 + mt * 16 + (ln >> 4) * 4 + r, n = n0 + nb * 16 + (ln & 15);
    if (m >= a.M || n >= a.N) continue;
    if (a.S == 1) sk_store(a, m, n, sk_epilogue(v, n, a));
    else a.ws[((long)s * a.M + m) * a.N + n] = v;
  }
}

__global__ __launch_bounds__(256) void skinny_reduce_kernel(SkArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.M * a.N) return;
  const int m = (int)(i / a.N), n = (int)(i % a.N);
  float v = 0.f;
  for (int s = 0; s < a.S; ++s) v += a.ws[(long)s * a.M * a.N + i];
  sk_store(a, m, n, sk_epilogue(v, n, a));
}

// ------------------------------------------------------------------------------------------------ decode attention
struct DecArgs {
  const bf16_t* q;
  const bf16_t* knew;
  const bf16_t* vnew;
  bf16_t* Kc;
  bf16_t* Vc;
  bf16_t* o;
  float* ws;
  long q_stride, k_stride, v_stride, o_stride;
  int H, Lmax, p, S, chunk;
  const int64_t* pos_dev;   // the device-position form (AT): p, S and chunk are derived in the kernel from *pos_dev, cap = the splits ws holds
  int cap;
};

// the device-position form: every workgroup reads the position and plans the split itself (decode_plan.h); false: nothing to do (a position outside
// [0, Lmax), which stores nothing)
__device__ __forceinline__ bool dec_plan_at(DecArgs& a) {
  const long p = *a.pos_dev;
  if (p < 0 || p >= a.Lmax) return false;
  const DecodePlan pl = decode_plan(p + 1, (long)gridDim.x, (long)a.cap);
  a.p = (int)p;
  a.S = (int)pl.S;
  a.chunk = (int)pl.chunk;
  return true;
}

constexpr int DEC_U = 4;   // keys per lane group in flight

template <int D, bool AT>
__global__ __launch_bounds__(256) void attn_decode_kernel(DecArgs a) {
  constexpr int G = D / 8;          // lanes per key (16 B each)
  constexpr int KPW = 64 / G;       // keys per wave per load round
  constexpr int NG = 4 * KPW;       // lane groups per block
  __shared__ float sm_acc[NG * D];
  __shared__ float sm_m[NG], sm_l[NG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, c = lane % G;
  const int grp = wave * KPW + g;
  const int bh = blockIdx.x, s = blockIdx.y;
  if (AT) {   // the grid is (B H, S bound): the splits past this position's S leave at once (block-uniform, before any barrier)
    if (!dec_plan_at(a) || s >= a.S) return;
  }
  const int b = bh / a.H, h = bh % a.H;
  const long d = (long)a.H * D;
  const int lo = s * a.chunk, hi = min(a.p + 1, lo + a.chunk);
  const long cache_row0 = (long)b * a.Lmax * d + h * D + c * 8;

  const uint4 qv = *(const uint4*)(a.q + b * a.q_stride + h * D + c * 8);
  const uint4 knv = *(const uint4*)(a.knew + b * a.k_stride + h * D + c * 8);
  const uint4 vnv = *(const uint4*)(a.vnew + b * a.v_stride + h * D + c * 8);
  if (s == a.S - 1 && threadIdx.x < G) {   // cache append: slot p of this (b, h), written by the one split that reads key p (from knew / vnew)
    *(uint4*)(a.Kc + cache_row0 + (long)a.p * d) = knv;
    *(uint4*)(a.Vc + cache_row0 + (long)a.p * d) = vnv;
  }
  float qf[8];
  {
    const bf16_t* qe = (const bf16_t*)&qv;
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[i] = bf2f(qe[i]);
  }
  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;

  for (int base = lo; base < hi; base += NG * DEC_U) {
    uint4 kk[DEC_U], vv[DEC_U];
    int js[DEC_U];
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const int j = base + u * NG + grp;
      js[u] = j;
      const int jc = min(j, a.p - 1 < 0 ? 0 : a.p - 1);   // (clamped address for keys outside [lo, hi) and for key p; their values are not used)
      const long off = cache_row0 + (long)jc * d;
      kk[u] = (j < hi && j != a.p) ? *(const uint4*)(a.Kc + off) : knv;
      vv[u] = (j < hi && j != a.p) ? *(const uint4*)(a.Vc + off) : vnv;
    }
    float sc[DEC_U];
    float mx = m;
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const bf16_t* ke = (const bf16_t*)&kk[u];
      float t = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) t += qf[i] * bf2f(ke[i]);
#pragma unroll
      for (int o = 1; o < G; o <<= 1) t += __shfl_xor(t, o, 64);
      sc[u] = js[u] < hi ? t : -INFINITY;
      mx = fmaxf(mx, sc[u]);
    }
    if (mx == -INFINITY) continue;
    const float scale = __builtin_amdgcn_exp2f(m - mx);   // (m = -inf: 0)
    l *= scale;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= scale;
#pragma unroll
    for (int u = 0; u < DEC_U; ++u) {
      const float pu = __builtin_amdgcn_exp2f(sc[u] - mx);
      l += pu;
      const bf16_t* ve = (const bf16_t*)&vv[u];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += pu * bf2f(ve[i]);
    }
    m = mx;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) sm_acc[grp * D + c * 8 + i] = acc[i];
  if (c == 0) {
    sm_m[grp] = m;
    sm_l[grp] = l;
  }
  __syncthreads();
  if (threadIdx.x < D) {
    const int t = threadIdx.x;
    float M = -INFINITY;
    for (int gi = 0; gi < NG; ++gi) M = fmaxf(M, sm_m[gi]);
    float L = 0.f, A = 0.f;
    for (int gi = 0; gi < NG; ++gi) {
      if (sm_m[gi] == -INFINITY) continue;
      const float wgt = __builtin_amdgcn_exp2f(sm_m[gi] - M);
      L += wgt * sm_l[gi];
      A += wgt * sm_acc[gi * D + t];
    }
    if (a.S == 1) {
      a.o[b * a.o_stride + h * D + t] = f2bf(A / L);
    } else {
      float* w = a.ws + ((long)bh * a.S + s) * (D + 2);
      w[2 + t] = A;
      if (t == 0) {
        w[0] = M;
        w[1] = L;
      }
    }
  }
}

template <int D, bool AT>
__global__ __launch_bounds__(D > 128 ? D : 128) void attn_decode_combine_kernel(DecArgs a) {
  const int bh = blockIdx.x, t = threadIdx.x;
  if (t >= D) return;
  if (AT) {   // launched always: with one split the first launch has written o itself
    if (!dec_plan_at(a) || a.S == 1) return;
  }
  const int b = bh / a.H, h = bh % a.H;
  const float* w = a.ws + (long)bh * a.S * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < a.S; ++s) M = fmaxf(M, w[s * (D + 2)]);
  float L = 0.f, A = 0.f;
  for (int s = 0; s < a.S; ++s) {
    const float wgt = __builtin_amdgcn_exp2f(w[s * (D + 2)] - M);
    L += wgt * w[s * (D + 2) + 1];
    A += wgt * w[s * (D + 2) + 2 + t];
  }
  a.o[b * a.o_stride + h * D + t] = f2bf(A / L);
}

// ------------------------------------------------------------------------------------------------ AR token choice
struct ArArgs {
  const bf16_t* logits;
  const bf16_t* logits_u;
  const float* w;
  const int64_t* modality;
  const float* g;
  int64_t* x;
  const int64_t* x0;
  const uint8_t* unmask;
  int64_t* next_ids;
  long ld, ldg, g_col0, ldx, ldm, pos, step, V, Vt, mask_id;
  uint64_t seed;
  int R, restrict_modality;
  const int64_t* pos_dev;   // the device-position form (AT): pos = i + 1, step = i, g_col0 = i V with i = *pos_dev
};

__device__ __forceinline__ bool ar_better(float v, long i, float bv, long bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ float gumbel_of(uint32_t r) {
  // u = ((r >> 8) + 0.5) 2^-24 in (0, 1).  x + 0.5 has 25 bits for x >= 2^23 and fp32 rounds it to an integer (u = 1 and a Gumbel of +inf at the top of the
  // grid), so the upper half is held as 1 - u = ((2^24 - 1 - x) + 0.5) 2^-24, which is exact, and -log(u) = -log1p(-(1 - u)).
  const uint32_t x = r >> 8;
  const float e = x < (1u << 23) ? -__logf(((float)x + 0.5f) * (1.0f / 16777216.0f)) : -log1pf(-(((float)(0xFFFFFFu - x) + 0.5f) * (1.0f / 16777216.0f)));
  return -__logf(e);
}

template <bool AT>
__global__ __launch_bounds__(512) void ar_sample_rows_kernel(ArArgs a) {
  __shared__ float sv[8];
  __shared__ long si[8];
  if (AT) {   // (block-uniform, before any barrier) a position whose column, modality column or noise columns do not exist: nothing is stored
    const long i = *a.pos_dev;
    if (i < 0 || i + 1 >= a.ldx || (a.restrict_modality && i + 1 >= a.ldm) || (a.g && (i + 1) * a.V > a.ldg)) return;
    a.pos = i + 1, a.step = i, a.g_col0 = i * a.V;
  }
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const bf16_t* lr = a.logits + (long)b * a.ld;
  const bf16_t* lu = a.logits_u ? a.logits_u + (long)b * a.ld : nullptr;
  const float w = a.logits_u ? *a.w : 0.f;
  const int img = a.restrict_modality ? (a.modality[(long)b * a.ldm + a.pos] == 1) : -1;
  const uint64_t key = a.seed ^ ((uint64_t)(a.step + 1) * 0x9E3779B97F4A7C15ull);
  float bv = -INFINITY;
  long bi = 0x7fffffffffffffffL;
  for (long v0 = (long)t * 8; v0 < a.V; v0 += 512 * 8) {
    const uint4 raw = *(const uint4*)(lr + v0);
    uint4 rawu = make_uint4(0, 0, 0, 0);
    if (lu) rawu = *(const uint4*)(lu + v0);
    uint32_t rnd[8];
    if (!a.g) {
      const uint4 r0 = udm::philox4x32(key, ((uint64_t)b << 40) | (uint64_t)(v0 >> 2));
      const uint4 r1 = udm::philox4x32(key, ((uint64_t)b << 40) | (uint64_t)((v0 >> 2) + 1));
      rnd[0] = r0.x, rnd[1] = r0.y, rnd[2] = r0.z, rnd[3] = r0.w, rnd[4] = r1.x, rnd[5] = r1.y, rnd[6] = r1.z, rnd[7] = r1.w;
    }
    const bf16_t* le = (const bf16_t*)&raw;
    const bf16_t* ue = (const bf16_t*)&rawu;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long v = v0 + i;
      if (v >= a.V || v == a.mask_id) continue;
      if (img >= 0 && (img ? v < a.Vt : v >= a.Vt)) continue;
      float z = bf2f(le[i]);
      if (lu) z = (1.f + w) * z - w * bf2f(ue[i]);
      z += a.g ? a.g[(long)b * a.ldg + a.g_col0 + v] : gumbel_of(rnd[i]);
      if (ar_better(z, v, bv, bi)) bv = z, bi = v;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const long oi = __shfl_xor(bi, o, 64);
    if (ar_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if ((t & 63) == 0) {
    sv[t >> 6] = bv;
    si[t >> 6] = bi;
  }
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < 8; ++i)
      if (ar_better(sv[i], si[i], bv, bi)) bv = sv[i], bi = si[i];
    if (bi == 0x7fffffffffffffffL) bi = 0;   // (no admissible id: cannot happen for V > 1 without NaN logits)
    const long at = (long)b * a.ldx + a.pos;
    const bool keep = a.unmask && a.unmask[at];
    const int64_t val = keep ? a.x0[at] : (int64_t)bi;
    a.x[at] = val;
    if (a.next_ids) {
      a.next_ids[b] = val;
      if (a.logits_u) a.next_ids[a.R + b] = keep ? a.mask_id : val;   // the unconditional half: where(x0_unmask, mask, x)
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int udm_gemm_skinny_bf16(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldc, int out_f32,
                                    int epilogue, const float* bias, float* ws, int64_t ws_elems, hipStream_t stream) {
  UDM_CHECK_ARG(A && W && C, "udm_gemm_skinny_bf16: null pointer");
  UDM_CHECK_ARG(M >= 1 && M <= 128 && N >= 1 && K >= 32 && K % 32 == 0, "udm_gemm_skinny_bf16: bad shape M=%ld N=%ld K=%ld (1 <= M <= 128, K %% 32 == 0)",
                (long)M, (long)N, (long)K);
  UDM_CHECK_ARG(lda >= K && ldw >= K && ldc >= N && lda % 8 == 0 && ldw % 8 == 0, "udm_gemm_skinny_bf16: bad leading dimensions");
  UDM_CHECK_ARG(al16(A) && al16(W) && al16(C) && (!ws || al16(ws)) && (!bias || al16(bias)), "udm_gemm_skinny_bf16: operands must be 16-byte aligned");
  UDM_CHECK_ARG(epilogue == UDM_EPI_NONE || epilogue == UDM_EPI_BIAS || epilogue == UDM_EPI_BIAS_GELU, "udm_gemm_skinny_bf16: epilogue %d not supported", epilogue);
  UDM_CHECK_ARG(epilogue == UDM_EPI_NONE || bias, "udm_gemm_skinny_bf16: the epilogue needs a bias");
  UDM_CHECK_ARG(N < (1L << 30) && K < (1L << 30), "udm_gemm_skinny_bf16: shape too large");
  // K split over workgroups until about two workgroups per CU stream (each slice >= 128 deep, the partial slabs must fit ws): skinny_plan.h
  const SkinnyPlan pl = skinny_plan(M, N, K, ws != nullptr, ws_elems);
  const int S = (int)pl.S;
  SkArgs a{(const bf16_t*)A, (const bf16_t*)W, C, ws, bias, (long)lda, (long)ldw, (long)ldc, (int)M, (int)N, (int)K, (int)pl.kslice, S, out_f32, epilogue};
  const dim3 grid((unsigned)pl.nblk, (unsigned)S);
  if (M <= 64) {
    switch ((int)((M + 15) / 16)) {
      case 1: hipLaunchKernelGGL(skinny_gemm_kernel<1>, grid, dim3(256), 0, stream, a); break;
      case 2: hipLaunchKernelGGL(skinny_gemm_kernel<2>, grid, dim3(256), 0, stream, a); break;
      case 3: hipLaunchKernelGGL(skinny_gemm_kernel<3>, grid, dim3(256), 0, stream, a); break;
      default: hipLaunchKernelGGL(skinny_gemm_kernel<4>, grid, dim3(256), 0, stream, a); break;
    }
  } else {   // rows [0, 64) and [64, M) in one workgroup, the weights loaded once for both
    switch ((int)((M - 64 + 15) / 16)) {
      case 1: hipLaunchKernelGGL(skinny_gemm2_kernel<1>, grid, dim3(256), 0, stream, a); break;
      case 2: hipLaunchKernelGGL(skinny_gemm2_kernel<2>, grid, dim3(256), 0, stream, a); break;
      case 3: hipLaunchKernelGGL(skinny_gemm2_kernel<3>, grid, dim3(256), 0, stream, a); break;
      default: hipLaunchKernelGGL(skinny_gemm2_kernel<4>, grid, dim3(256), 0, stream, a); break;
    }
  }
  UDM_CHECK_LAUNCH("udm_gemm_skinny_bf16");
  if (S > 1) {
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, stream, a);
    UDM_CHECK_LAUNCH("udm_gemm_skinny_bf16 (reduce)");
  }
  return 0;
}

namespace {

// the shape checks both forms of the decode attention share (`p` apart); `name` prefixes the message
int dec_check(const char* name, const void* q, const void* k_new, const void* v_new, const void* k_cache, const void* v_cache, const void* o, const float* ws,
              int64_t B, int64_t H, int64_t D, int64_t Lmax, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t o_stride) {
  UDM_CHECK_ARG(q && k_new && v_new && k_cache && v_cache && o, "%s: null pointer", name);
  UDM_CHECK_ARG(D == 32 || D == 64 || D == 128 || D == 256, "%s: head dim %ld (32 / 64 / 128 / 256)", name, (long)D);
  UDM_CHECK_ARG(B >= 1 && H >= 1 && Lmax >= 1 && Lmax < (1L << 30) && B * H < (1L << 30), "%s: bad shape B=%ld H=%ld Lmax=%ld", name, (long)B, (long)H, (long)Lmax);
  UDM_CHECK_ARG(q_stride % 8 == 0 && k_stride % 8 == 0 && v_stride % 8 == 0 && o_stride % 8 == 0 && q_stride >= H * D && k_stride >= H * D &&
                    v_stride >= H * D && o_stride >= H * D, "%s: bad row strides", name);
  UDM_CHECK_ARG(al16(q) && al16(k_new) && al16(v_new) && al16(k_cache) && al16(v_cache) && al16(o) && (!ws || al16(ws)), "%s: operands must be 16-byte aligned", name);
  return 0;
}

template <bool AT>
void dec_launch(int64_t D, dim3 grid, const DecArgs& a, hipStream_t stream) {
  switch (D) {
    case 32: hipLaunchKernelGGL((attn_decode_kernel<32, AT>), grid, dim3(256), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((attn_decode_kernel<64, AT>), grid, dim3(256), 0, stream, a); break;
    case 256: hipLaunchKernelGGL((attn_decode_kernel<256, AT>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((attn_decode_kernel<128, AT>), grid, dim3(256), 0, stream, a); break;
  }
}

template <bool AT>
void dec_launch_combine(int64_t D, unsigned BH, const DecArgs& a, hipStream_t stream) {
  switch (D) {
    case 32: hipLaunchKernelGGL((attn_decode_combine_kernel<32, AT>), dim3(BH), dim3(128), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((attn_decode_combine_kernel<64, AT>), dim3(BH), dim3(128), 0, stream, a); break;
    case 256: hipLaunchKernelGGL((attn_decode_combine_kernel<256, AT>), dim3(BH), dim3(256), 0, stream, a); break;   // one thread per output column
    default: hipLaunchKernelGGL((attn_decode_combine_kernel<128, AT>), dim3(BH), dim3(128), 0, stream, a); break;
  }
}

}  // namespace

extern "C" int udm_attention_decode(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o, float* ws, int64_t ws_elems,
                                    int64_t B, int64_t H, int64_t D, int64_t Lmax, int64_t p, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                    int64_t o_stride, hipStream_t stream) {
  if (int rc = dec_check("udm_attention_decode", q, k_new, v_new, k_cache, v_cache, o, ws, B, H, D, Lmax, q_stride, k_stride, v_stride, o_stride)) return rc;
  UDM_CHECK_ARG(p >= 0 && p < Lmax, "udm_attention_decode: bad shape B=%ld H=%ld Lmax=%ld p=%ld", (long)B, (long)H, (long)Lmax, (long)p);
  const long BH = B * H;
  // splits: about two workgroups per CU over B H, at least 64 keys each, at most 32, bounded by ws (decode_plan.h)
  const long cap = ws ? ws_elems / (BH * (D + 2)) : 1;
  const DecodePlan pl = decode_plan(p + 1, BH, cap);
  DecArgs a{(const bf16_t*)q, (const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_cache, (bf16_t*)v_cache, (bf16_t*)o, ws, (long)q_stride, (long)k_stride,
            (long)v_stride, (long)o_stride, (int)H, (int)Lmax, (int)p, (int)pl.S, (int)pl.chunk, nullptr, 0};
  dec_launch<false>(D, dim3((unsigned)BH, (unsigned)pl.S), a, stream);
  UDM_CHECK_LAUNCH("udm_attention_decode");
  if (pl.S > 1) {
    dec_launch_combine<false>(D, (unsigned)BH, a, stream);
    UDM_CHECK_LAUNCH("udm_attention_decode (combine)");
  }
  return 0;
}

extern "C" int udm_attention_decode_at(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, void* o, float* ws, int64_t ws_elems,
                                       int64_t B, int64_t H, int64_t D, int64_t Lmax, const int64_t* pos_dev, int64_t q_stride, int64_t k_stride,
                                       int64_t v_stride, int64_t o_stride, hipStream_t stream) {
  if (int rc = dec_check("udm_attention_decode_at", q, k_new, v_new, k_cache, v_cache, o, ws, B, H, D, Lmax, q_stride, k_stride, v_stride, o_stride)) return rc;
  UDM_CHECK_ARG(pos_dev && ((uintptr_t)pos_dev & 7) == 0, "udm_attention_decode_at: the position must be an aligned device int64");
  const long BH = B * H;
  long cap = ws ? ws_elems / (BH * (D + 2)) : 1;
  cap = cap < 1 ? 1 : (cap > 32 ? 32 : cap);
  // the grid holds the S of every position below Lmax (S is not monotone in the position: decode_plan.h); both launches always, the kernels decide
  const long Sb = decode_plan_s_bound(BH, Lmax, cap);
  DecArgs a{(const bf16_t*)q, (const bf16_t*)k_new, (const bf16_t*)v_new, (bf16_t*)k_cache, (bf16_t*)v_cache, (bf16_t*)o, ws, (long)q_stride, (long)k_stride,
            (long)v_stride, (long)o_stride, (int)H, (int)Lmax, 0, 1, 64, pos_dev, (int)cap};
  dec_launch<true>(D, dim3((unsigned)BH, (unsigned)Sb), a, stream);
  UDM_CHECK_LAUNCH("udm_attention_decode_at");
  dec_launch_combine<true>(D, (unsigned)BH, a, stream);
  UDM_CHECK_LAUNCH("udm_attention_decode_at (combine)");
  return 0;
}

extern "C" int udm_ar_sample_rows(const void* logits, const void* logits_uncond, const float* w, int64_t ld, const int64_t* modality, int64_t ldm, const float* g,
                                  int64_t ldg, int64_t g_col0, uint64_t seed, int64_t step, int64_t* x, int64_t ldx, const int64_t* x0, const void* x0_unmask,
                                  int64_t pos, int64_t* next_ids, int64_t R, int64_t V, int64_t Vt, int64_t mask_id, int restrict_modality, hipStream_t stream) {
  UDM_CHECK_ARG(logits && x, "udm_ar_sample_rows: null pointer");
  UDM_CHECK_ARG(R >= 1 && V >= 1 && ld >= V && ld % 8 == 0 && pos >= 0 && pos < ldx, "udm_ar_sample_rows: bad shape R=%ld V=%ld ld=%ld pos=%ld", (long)R, (long)V,
                (long)ld, (long)pos);
  UDM_CHECK_ARG(!logits_uncond || w, "udm_ar_sample_rows: guidance needs the weight");
  UDM_CHECK_ARG(!restrict_modality || (modality && ldm > pos && Vt > 0 && Vt < V), "udm_ar_sample_rows: the restriction needs the modality map and 0 < Vt < V");
  UDM_CHECK_ARG(!x0_unmask || x0, "udm_ar_sample_rows: x0_unmask needs x0");
  UDM_CHECK_ARG(!g || (ldg >= g_col0 + V && g_col0 >= 0), "udm_ar_sample_rows: bad noise layout");
  UDM_CHECK_ARG(al16(logits) && (!logits_uncond || al16(logits_uncond)) && (!w || al16(w)) && (!modality || al16(modality)) && (!g || al16(g)) && al16(x) &&
                    (!x0 || al16(x0)) && (!x0_unmask || al16(x0_unmask)) && (!next_ids || al16(next_ids)),
                "udm_ar_sample_rows: operands must be 16-byte aligned");
  ArArgs a{(const bf16_t*)logits, (const bf16_t*)logits_uncond, w, modality, g, x, x0, (const uint8_t*)x0_unmask, next_ids, (long)ld, (long)ldg, (long)g_col0,
           (long)ldx, (long)ldm, (long)pos, (long)step, (long)V, (long)Vt, (long)mask_id, seed, (int)R, restrict_modality, nullptr};
  hipLaunchKernelGGL(ar_sample_rows_kernel<false>, dim3((unsigned)R), dim3(512), 0, stream, a);
  UDM_CHECK_LAUNCH("udm_ar_sample_rows");
  return 0;
}

extern "C" int udm_ar_sample_rows_at(const void* logits, const void* logits_uncond, const float* w, int64_t ld, const int64_t* modality, int64_t ldm,
                                     const float* g, int64_t ldg, uint64_t seed, int64_t* x, int64_t ldx, const int64_t* x0, const void* x0_unmask,
                                     const int64_t* pos_dev, int64_t* next_ids, int64_t R, int64_t V, int64_t Vt, int64_t mask_id, int restrict_modality,
                                     hipStream_t stream) {
  UDM_CHECK_ARG(logits && x && pos_dev && ((uintptr_t)pos_dev & 7) == 0, "udm_ar_sample_rows_at: null pointer (the position must be an aligned device int64)");
  UDM_CHECK_ARG(R >= 1 && V >= 1 && ld >= V && ld % 8 == 0 && ldx >= 1, "udm_ar_sample_rows_at: bad shape R=%ld V=%ld ld=%ld ldx=%ld", (long)R, (long)V, (long)ld,
                (long)ldx);
  UDM_CHECK_ARG(!logits_uncond || w, "udm_ar_sample_rows_at: guidance needs the weight");
  UDM_CHECK_ARG(!restrict_modality || (modality && ldm >= 1 && Vt > 0 && Vt < V), "udm_ar_sample_rows_at: the restriction needs the modality map and 0 < Vt < V");
  UDM_CHECK_ARG(!x0_unmask || x0, "udm_ar_sample_rows_at: x0_unmask needs x0");
  UDM_CHECK_ARG(!g || ldg >= V, "udm_ar_sample_rows_at: bad noise layout");
  UDM_CHECK_ARG(al16(logits) && (!logits_uncond || al16(logits_uncond)) && (!w || al16(w)) && (!modality || al16(modality)) && (!g || al16(g)) && al16(x) &&
                    (!x0 || al16(x0)) && (!x0_unmask || al16(x0_unmask)) && (!next_ids || al16(next_ids)),
                "udm_ar_sample_rows_at: operands must be 16-byte aligned");
  ArArgs a{(const bf16_t*)logits, (const bf16_t*)logits_uncond, w, modality, g, x, x0, (const uint8_t*)x0_unmask, next_ids, (long)ld, (long)ldg, 0L,
           (long)ldx, (long)ldm, 0L, 0L, (long)V, (long)Vt, (long)mask_id, seed, (int)R, restrict_modality, pos_dev};
  hipLaunchKernelGGL(ar_sample_rows_kernel<true>, dim3((unsigned)R), dim3(512), 0, stream, a);
  UDM_CHECK_LAUNCH("udm_ar_sample_rows_at");
  return 0;
}

// ------------------------------------------------------------------------------------------------ position-dependent small operands of a captured step
namespace {

struct StageArgs {
  const int64_t* pos_dev;
  const int64_t* mod_cols;   // [L, Bp] (nullable)
  int64_t* mod_row;          // [Bp]
  const float* cos;          // [L, rope_row] (nullable)
  const float* sin;
  float* cos_row;            // [rope_row]
  float* sin_row;
  long L, Bp, rope_row;
};

__global__ __launch_bounds__(256) void decode_stage_kernel(StageArgs a) {
  const long p = *a.pos_dev;
  if (p < 0 || p >= a.L) return;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (a.mod_cols && t < a.Bp) a.mod_row[t] = a.mod_cols[p * a.Bp + t];
  if (a.cos && t < a.rope_row) {
    a.cos_row[t] = a.cos[p * a.rope_row + t];
    a.sin_row[t] = a.sin[p * a.rope_row + t];
  }
}

__global__ void counter_add_kernel(int64_t* c, int64_t delta) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *c += delta;
}

}  // namespace

extern "C" int udm_decode_stage(const int64_t* pos_dev, const int64_t* mod_cols, int64_t* mod_row, int64_t Bp, const float* cos, const float* sin, float* cos_row,
                                float* sin_row, int64_t rope_row, int64_t L, hipStream_t stream) {
  UDM_CHECK_ARG(pos_dev && ((uintptr_t)pos_dev & 7) == 0, "udm_decode_stage: the position must be an aligned device int64");
  UDM_CHECK_ARG(L >= 1 && L < (1L << 30), "udm_decode_stage: bad table length L=%ld", (long)L);
  UDM_CHECK_ARG(!mod_cols || (mod_row && Bp >= 1 && Bp < (1L << 20)), "udm_decode_stage: the modality column needs its [Bp] buffer");
  UDM_CHECK_ARG((cos == nullptr) == (sin == nullptr) && (!cos || (cos_row && sin_row && rope_row >= 1 && rope_row < (1L << 24))),
                "udm_decode_stage: the rotary rows need both tables and both one-row buffers");
  const long n = (mod_cols ? Bp : 0) > (cos ? rope_row : 0) ? (long)Bp : (cos ? (long)rope_row : 0);
  if (n == 0) return 0;
  StageArgs a{pos_dev, mod_cols, mod_row, cos, sin, cos_row, sin_row, (long)L, (long)Bp, (long)rope_row};
  hipLaunchKernelGGL(decode_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  UDM_CHECK_LAUNCH("udm_decode_stage");
  return 0;
}

extern "C" int udm_counter_add(int64_t* c, int64_t delta, hipStream_t stream) {
  UDM_CHECK_ARG(c && ((uintptr_t)c & 7) == 0, "udm_counter_add: the counter must be an aligned device int64");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, stream, c, delta);
  UDM_CHECK_LAUNCH("udm_counter_add");
  return 0;
}
