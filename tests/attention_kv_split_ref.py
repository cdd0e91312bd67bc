"""The key-split form of tests/attention_ref64.py::emulate_fwd_tiled (CPU only): what udm_attention_fwd_kv_split computes with S > 1 splits.

Every split walks its contiguous range of 64-key tiles (attn_kv_split_range of csrc/attention_plan.h: balanced, the longer ranges first, the last one carries the
Lk tail) with the kernels' online softmax and lazy reference exponent, and leaves (m, l, unnormalised O) in fp32; the combine forms M = max_s m_s and
O = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s in the order s = 0 .. S - 1 with ONE rounding to bf16, lse2 = M + log2 of the denominator.
`mutant` seeds the three errors the comparator must reject: "dropped_split" (the combine leaves the last split out), "unweighted" (a combine without the
2^(m_s - M) weights) and "range_off_by_one" (the second split starts one tile late: a tile nobody walks)."""
import torch

import attention_ref64 as R

TILE = 64


def split_ranges(Lk, S):
    """[(first tile, end tile)] of the S splits; S must not exceed the tile count"""
    T = -(-Lk // TILE)
    assert 1 <= S <= T
    base, rem = divmod(T, S)
    out = []
    for s in range(S):
        b = s * base + min(s, rem)
        out.append((b, b + base + (1 if s < rem else 0)))
    return out


def clamp_splits(Lk, S):
    return max(1, min(S, -(-Lk // TILE), 32))


def _partial(s_all, vf, t0, t1, Lk, lazy):
    """the online softmax of emulate_fwd_tiled over the tiles [t0, t1): (m [.., 1], l [.., 1], acc [.., D]) in fp32"""
    B, H, L, _ = s_all.shape
    D = vf.shape[-1]
    m = torch.full((B, H, L, 1), float("-inf"))
    l = torch.zeros(B, H, L, 1)
    acc = torch.zeros(B, H, L, D)
    for t in range(t0, t1):
        k0, k1 = t * TILE, min((t + 1) * TILE, Lk)
        s = s_all[..., k0:k1]
        mloc = s.max(-1, keepdim=True).values
        m_new = torch.where(mloc > m + lazy, torch.maximum(m, mloc), m)
        alpha = torch.exp2(m - torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new))
        alpha = torch.where(torch.isinf(m), torch.zeros_like(alpha), alpha)
        l, acc, m = l * alpha, acc * alpha, m_new
        pr = torch.exp2(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        l = l + pr.sum(-1, keepdim=True)
        acc = acc + R._bf(pr) @ vf[..., k0:k1, :]
    return m, l, acc


def emulate_fwd_tiled_split(q, k, v, *, prescaled, splits, lazy=8.0, mutant=None):
    """q [B, H, Lq, D], k / v [B, H, Lk, D] (bf16) -> (O bf16-valued fp32, lse2 fp32) through `splits` key splits (lowered to the tile count and to 32)"""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    c2, _ = R.score_scales(D, prescaled)
    s_all = R._scores32(q, k, c2, None)
    vf = v.float()
    S = clamp_splits(Lk, splits)
    ranges = split_ranges(Lk, S)
    if mutant == "range_off_by_one" and S > 1:
        ranges[1] = (ranges[1][0] + 1, ranges[1][1])
    parts = [_partial(s_all, vf, t0, t1, Lk, lazy) for t0, t1 in ranges]
    if mutant == "dropped_split":
        parts = parts[:-1]
    M = torch.stack([p[0] for p in parts]).max(0).values
    num = torch.zeros(B, H, Lq, D)
    den = torch.zeros(B, H, Lq, 1)
    for m, l, acc in parts:
        w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - torch.where(torch.isinf(M), torch.zeros_like(M), M)))
        if mutant == "unweighted":
            w = torch.ones_like(w)
        num = num + w * acc
        den = den + w * l
    live = den > 0
    safe = torch.where(live, den, torch.ones_like(den))
    o = R._bf(torch.where(live, num / safe, torch.zeros_like(num)))
    lse = torch.where(live, M + torch.log2(safe), torch.full_like(den, float("inf")))
    return o, lse.squeeze(-1)
