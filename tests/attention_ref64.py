"""fp64 attention with per-row error scales, two bf16 flash-attention emulations, and adversarial input families (CPU only).

The reference of tests/test_gpu_attention_rowwise.py (GPU) and tests/test_attention_ref64.py (CPU); the split follows optim_ref.py / optim_cases.py.

Conventions: operands are [B, H, L, D] tensors holding bf16 values.  Scores are BASE-2 exponents, s2 = q k c2 with c2 = 1 for a pre-scaled q
(UDM_ATTN_Q_PRESCALED: q holds q log2(e) / sqrt(D)) and c2 = log2(e) / sqrt(D) otherwise; lse2 = log2(sum_j 2^s2) as the kernels store it.  The backward is the
closed form (dS wrt the natural-log scores): dV = (P o Z~)^T dO, dP = dO V^T, delta = rowsum(dO o O), dS = P o (Z~ o dP - delta), dQ = dS K cb, dK = dS^T Q cb with
cb = 1 / sqrt(D), or ln 2 for a pre-scaled q (the gradient wrt the STORED q).  Z~ = keep / (1 - p) is the dropout mask of include/unidisc_hip.h (1 without dropout).

Row scales: the magnitude sums the rounding errors of a bf16 flash attention are relative to,
    sc_O  = (P o Z~) |V|                      sc_dV = (P o Z~)^T |dO|
    dbar_i = sum_d |dO_id| sc_O[i, d]         (NOT |delta|: the true delta cancels, the error of a delta computed from a rounded O does not)
    W = P o (Z~ o |dP| + dbar)                sc_dQ = W |K| cb,   sc_dK = W^T |Q| cb
and the row statistic  e_r = ||got_r - ref_r||_2 / max(||sc_r||_2, 2^-60 max_r ||sc_r||_2)  over the D elements of one (b, h, row).

Bounds, with u = 2^-8 the bf16 unit roundoff (every rounding of the chain is at most u relative to a quantity the scale dominates):
    O, dV: two roundings (P, the output)                   max_r e_r <= 2 u
    dQ, dK: three (O inside delta, dS, the output)         max_r e_r <= 3 u
    lse2: |err| <= (D + 8) 2^-24 max_j(|q_i|^T |k_j| c2) + 2^-20   (fp32 dot product, plus the log)
"""
import math

import numpy as np
import torch

import attn_prob_dropout_ref as dropref

U = 2.0 ** -8
BOUNDS = dict(o=2 * U, dv=2 * U, dq=3 * U, dk=3 * U)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
BF16 = torch.bfloat16

FAMILIES = ("gauss", "ramp_up", "ramp_down", "row_offset", "spikes", "pointer", "pointer_onehot")
FAMILIES_SHORT = ("gauss", "ramp_up", "row_offset", "pointer")
DECODE_FAMILIES = ("ramp_up", "ramp_down", "spikes", "pointer")
ONEHOT_ROWS = (0, 63, 64, 127, 128, 255, 256, -1)


def score_scales(D, prescaled):
    """(c2, cb): the forward's base-2 score scale and the factor the backward puts on dQ / dK"""
    return (1.0, LN2) if prescaled else (LOG2E / math.sqrt(D), 1.0 / math.sqrt(D))


def decode_codes(sample_ids):
    """mask codes (csrc/attention_common.h) -> (id, key class, query mask): the id is the sign-extended low 32 bits, bits 32-39 the key class, bits 40-47 the
    query mask; a zero class or mask field reads as 0xff ("all").  Raw sample ids decode to (id, 0xff, 0xff)."""
    code = torch.as_tensor(sample_ids).to(torch.int64)
    ids = ((code & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    kcls, qmask = (code >> 32) & 0xFF, (code >> 40) & 0xFF
    return ids, torch.where(kcls == 0, 0xFF, kcls), torch.where(qmask == 0, 0xFF, qmask)


PREDICATE_MUTANTS = ("ignore_class_bits", "swap_mask_and_class", "class4_visible", "padding_is_minus_one_only")


def pair_ok(sample_ids, mutant=None):
    """bool [B, L, L]: attn_pair_ok of every (query i, key j) - ids equal and >= 0 and (qmask_i & kclass_j) != 0 - or one of PREDICATE_MUTANTS, a wrong predicate"""
    ids, kcls, qmask = decode_codes(sample_ids)
    live = ids[:, :, None] != -1 if mutant == "padding_is_minus_one_only" else ids[:, :, None] >= 0
    same = (ids[:, :, None] == ids[:, None, :]) & live
    if mutant == "ignore_class_bits":
        return same
    if mutant == "swap_mask_and_class":          # the key's mask against the query's class
        return same & ((qmask[:, None, :] & kcls[:, :, None]) != 0)
    if mutant == "class4_visible":               # a class outside the known text / image bits reads as "every class" on the key side
        kcls = torch.where((kcls & 3) == 0, 0xFF, kcls)
    return same & ((qmask[:, :, None] & kcls[:, None, :]) != 0)


def visible(B, Lq, Lk, sample_ids=None, causal=False, mutant=None):
    """bool [B, 1, Lq, Lk] (True = query i sees key j), or None when every pair is visible.  `sample_ids` are mask codes, judged as attn_pair_ok does (pair_ok;
    padding is id < 0); `mutant` is for the tests that show a wrong predicate is noticed.  Causal: j <= i + (Lk - Lq) (the queries are the LAST Lq positions)."""
    ok = None
    if sample_ids is not None:
        ok = pair_ok(sample_ids, mutant)[:, None]
    if causal:
        tri = (torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + (Lk - Lq))[None, None]
        ok = tri.expand(B, 1, Lq, Lk) if ok is None else ok & tri
    return ok


def keep_scaled(seed, p, B, H, L):
    """Z~ = keep / (1 - p) as fp64 [B, H, L, L] (nominal p in fp32, as the kernels and torch take it)"""
    keep = torch.from_numpy(dropref.keep_mask(seed, p, B, H, L))
    return keep.double() * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ fp64 reference
def _ref_one(q, k, v, do, ok, zt, c2, cb):
    """one batch element: q [H, Lq, D], k / v [H, Lk, D], ok [1, Lq, Lk] or None, zt [H, Lq, Lk] or None"""
    s = q @ k.transpose(-1, -2) * c2
    if ok is not None:
        s = s.masked_fill(~ok, float("-inf"))
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m)                                   # rows that see no key (padding): P = 0, O = 0, lse2 = +inf
    e = torch.exp2(s - torch.where(dead, torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(dead, torch.ones_like(l), l)
    del s, e
    lse2 = torch.where(dead, torch.full_like(m, float("inf")), m + torch.log2(torch.where(dead, torch.ones_like(l), l))).squeeze(-1)
    aq, ak = q.abs(), k.abs()
    qk = aq @ ak.transpose(-1, -2)
    if ok is not None:
        qk = qk.masked_fill(~ok, 0.0)
    D = q.shape[-1]
    out = dict(lse2=lse2, lse_bound=(D + 8) * 2.0 ** -24 * qk.max(-1).values * c2 + 2.0 ** -20)
    del qk
    PZ = P if zt is None else P * zt
    out["o"] = PZ @ v
    out["sc_o"] = PZ @ v.abs()
    if do is None:
        return out
    out["dv"] = PZ.transpose(-1, -2) @ do
    out["sc_dv"] = PZ.transpose(-1, -2) @ do.abs()
    del PZ
    dP = do @ v.transpose(-1, -2)
    if zt is not None:
        dP = dP * zt
    delta = (do * out["o"]).sum(-1, keepdim=True)
    dbar = (do.abs() * out["sc_o"]).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out["dq"] = dS @ k * cb
    out["dk"] = dS.transpose(-1, -2) @ q * cb
    del dS
    W = P * (dP.abs() + dbar)
    del dP, P
    out["sc_dq"] = W @ ak * cb
    out["sc_dk"] = W.transpose(-1, -2) @ aq * cb
    return out


def attention_ref64(q, k, v, do=None, *, prescaled, sample_ids=None, causal=False, zt=None):
    """q [B, H, Lq, D], k / v [B, H, Lk, D], do like q (or None: forward only) -> dict of fp64 tensors o, lse2, lse_bound, sc_o (and dq, dk, dv, sc_dq, sc_dk, sc_dv)."""
    B, H, Lq, D = q.shape
    c2, cb = score_scales(D, prescaled)
    ok = visible(B, Lq, k.shape[2], sample_ids, causal)
    outs = []
    for b in range(B):
        outs.append(_ref_one(q[b].double(), k[b].double(), v[b].double(), None if do is None else do[b].double(), None if ok is None else ok[b],
                             None if zt is None else zt[b], c2, cb))
    return {key: torch.stack([o[key] for o in outs]) for key in outs[0]}


# ------------------------------------------------------------------------------------------------ metrics
def row_errors(got, ref, sc):
    """(max_r e_r, median_r e_r, (b, h, row) of the maximum) for [B, H, L, D] tensors"""
    num = (got.double() - ref).norm(dim=-1)
    den = sc.norm(dim=-1)
    den = den.clamp_min(2.0 ** -60 * float(den.max()))
    e = num / den
    e = torch.where(den > 0, e, torch.where(num > 0, float("inf"), 0.0).double())      # (nothing to be relative to: any deviation is an error)
    i = int(e.argmax())
    H, L = e.shape[1], e.shape[2]
    return float(e.reshape(-1)[i]), float(e.median()), (i // (H * L), i // L % H, i % L)


def lse_excess(got, ref):
    """max over live rows of |lse2 error| / its bound (<= 1 passes), the (b, h, row) of that maximum, and whether the dead rows (no visible key) hold +inf"""
    live = torch.isfinite(ref["lse2"])
    err = torch.where(live, (got.double() - ref["lse2"]).abs() / ref["lse_bound"], torch.zeros_like(ref["lse2"]))
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(err.argmax())
    H, L = err.shape[1], err.shape[2]
    dead_ok = bool((got[~live] == float("inf")).all())
    return float(err.reshape(-1)[i]), (i // (H * L), i // L % H, i % L), dead_ok


# ------------------------------------------------------------------------------------------------ bf16 flash-attention emulations (fp32 arithmetic)
def _bf(t):
    return t.to(BF16).float()


def _scores32(q, k, c2, ok):
    s = (q.float() @ k.float().transpose(-1, -2)) * c2
    return s if ok is None else s.masked_fill(~ok, float("-inf"))


def emulate_fwd_oneshot(q, k, v, *, prescaled, sample_ids=None, causal=False, keep=None, p=0.0, mutant=None):
    """FA2 rounding points in one shot: fp32 scores and lse, P -> bf16, fp32 accumulate, O -> bf16.  Returns (O bf16-valued fp32, lse2 fp32)."""
    B, H, L, D = q.shape
    c2, _ = score_scales(D, prescaled)
    s = _scores32(q, k, c2, visible(B, L, k.shape[2], sample_ids, causal, mutant))
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m)
    l = torch.exp2(s - torch.where(dead, torch.zeros_like(m), m)).sum(-1, keepdim=True)
    lse = torch.where(dead, torch.full_like(m, float("inf")), m + torch.log2(l))
    P = torch.where(dead, torch.zeros_like(s), torch.exp2(s - torch.where(dead, torch.zeros_like(lse), lse)))
    ks = 1.0
    if keep is not None:
        P = P * torch.as_tensor(keep).float()
        ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return _bf((_bf(P) @ v.float()) * ks), lse.squeeze(-1)


def emulate_fwd_tiled(q, k, v, *, prescaled, sample_ids=None, causal=False, keep=None, p=0.0, tile=64, lazy=8.0, mutant=None):
    """Online softmax over 64-key tiles with the kernels' lazy reference exponent: a row's exponent m moves (and its l, acc are rescaled) only when a score of
    the tile exceeds it by more than 2^8; p = 2^(s - m) may exceed 1 by 2^8.  P -> bf16 per tile, fp32 accumulate, O = bf16(acc / l)."""
    B, H, L, D = q.shape
    Lk = k.shape[2]
    c2, _ = score_scales(D, prescaled)
    s_all = _scores32(q, k, c2, visible(B, L, Lk, sample_ids, causal, mutant))
    vf = v.float()
    m = torch.full((B, H, L, 1), float("-inf"))
    l = torch.zeros(B, H, L, 1)
    acc = torch.zeros(B, H, L, D)
    for t0 in range(0, Lk, tile):
        s = s_all[..., t0:t0 + tile]
        mloc = s.max(-1, keepdim=True).values
        m_new = torch.where(mloc > m + lazy, torch.maximum(m, mloc), m)
        alpha = torch.exp2(m - torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new))
        alpha = torch.where(torch.isinf(m), torch.zeros_like(alpha), alpha)          # (nothing accumulated yet)
        l, acc, m = l * alpha, acc * alpha, m_new
        pr = torch.exp2(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        l = l + pr.sum(-1, keepdim=True)
        if keep is not None:
            pr = pr * torch.as_tensor(keep[..., t0:t0 + tile]).float()
        acc = acc + _bf(pr) @ vf[..., t0:t0 + tile, :]
    ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if keep is not None else 1.0
    live = l > 0
    inv = torch.where(live, ks / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(l))
    lse = torch.where(live, m + torch.log2(torch.where(live, l, torch.ones_like(l))), torch.full_like(l, float("inf")))
    return _bf(acc * inv), lse.squeeze(-1)


def emulate_bwd(q, k, v, o, do, lse, *, prescaled, sample_ids=None, causal=False, keep=None, p=0.0, mutant=None):
    """The backward every flash attention runs, from the forward's bf16 O and fp32 lse2: P = 2^(s - lse) and dS rounded to bf16 in front of their matrix products,
    delta from the rounded O, fp32 accumulate, bf16 outputs.  Returns dq, dk, dv (bf16-valued fp32)."""
    B, H, L, D = q.shape
    c2, cb = score_scales(D, prescaled)
    s = _scores32(q, k, c2, visible(B, L, k.shape[2], sample_ids, causal, mutant))
    lse = lse.unsqueeze(-1)
    dead = torch.isinf(lse)
    P = torch.where(dead, torch.zeros_like(s), torch.exp2(s - torch.where(dead, torch.zeros_like(lse), lse)))
    dof = do.float()
    dP = dof @ v.float().transpose(-1, -2)
    PZ, ks = P, 1.0
    if keep is not None:
        z = torch.as_tensor(keep).float()
        ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        PZ, dP = P * z, dP * z * ks
    delta = (dof * o.float()).sum(-1, keepdim=True)
    dv = _bf((_bf(PZ).transpose(-1, -2) @ dof) * ks)
    dS = _bf(P * (dP - delta))
    return _bf(dS @ k.float() * cb), _bf(dS.transpose(-1, -2) @ q.float() * cb), dv


# ------------------------------------------------------------------------------------------------ input families
def _pointer_map(L, gen, causal, sid_row):
    """pi: the key each query points at.  A permutation; inside the own document under sample ids.  Under the causal flag pi(i) <= i (a permutation with that
    property is the identity, so the causal map is a uniform draw from [0, i] and not injective: dV_j then sums the dO rows that point at j)."""
    if causal:
        return (torch.rand(L, generator=gen) * (torch.arange(L) + 1)).long().clamp_max(torch.arange(L))
    if sid_row is None:
        return torch.randperm(L, generator=gen)
    pi = torch.arange(L)
    for doc in torch.unique(sid_row).tolist():
        idx = (sid_row == doc).nonzero().squeeze(-1)
        pi[idx] = idx[torch.randperm(len(idx), generator=gen)]
    return pi


def spike_rows(L):
    """six key rows in late tiles (and at tile seams); positions that do not fit a short L are replaced by rows counted back from the end, never wrapped"""
    rows = {r for r in (70, 200, L // 2 - 1, L // 2 + 64, L - 65, L - 1) if 0 <= r < L}
    fill = L - 10
    while len(rows) < min(6, L):
        rows.add(fill % L)
        fill -= 9
    return sorted(rows)


def make_inputs(family, B, H, L, D, *, prescaled, causal=False, sample_ids=None, seed=0):
    """q, k, v, do: bf16 [B, H, L, D].  Built in base-2 score units (so that pre-scaled and plain calls see the same scores), then q is divided by c2 for a plain call.
    Head dimension D - 1 carries the family's structure, the others 1.2 randn (scores of sigma ~ 2)."""
    gen = torch.Generator().manual_seed(seed)
    c2, _ = score_scales(D, prescaled)
    q2 = 1.2 * torch.randn(B, H, L, D, generator=gen) * (LOG2E / math.sqrt(D))
    k = 1.2 * torch.randn(B, H, L, D, generator=gen)
    v = 1.2 * torch.randn(B, H, L, D, generator=gen)
    do = 1.2 * torch.randn(B, H, L, D, generator=gen)
    j = torch.arange(L, dtype=torch.float32)
    if family == "gauss":
        pass
    elif family == "ramp_up":          # +16 per 64-key tile: the reference exponent moves on EVERY tile
        q2[..., D - 1], k[..., D - 1] = 1.0, 0.25 * j
    elif family == "ramp_down":        # the exponent never moves after tile 0; P spans 2^(-L / 4)
        q2[..., D - 1], k[..., D - 1] = 1.0, 0.25 * (L - 1 - j)
    elif family == "row_offset":       # whole rows at -96 ... +96 (the generated forward's exponent starts at 0 and only rises: -96 is the side that matters)
        q2[..., D - 1], k[..., D - 1] = 32.0 * ((torch.arange(L) % 7) - 3).float(), 1.0
    elif family == "spikes":           # queries that share a wave disagree about the move
        k[:, :, spike_rows(L)] *= 6.0
    elif family in ("pointer", "pointer_onehot"):
        k = torch.where(torch.rand(B, H, L, D, generator=gen) < 0.5, -1.0, 1.0)
        for b in range(B):
            for h in range(H):
                pi = _pointer_map(L, gen, causal, None if sample_ids is None else torch.as_tensor(sample_ids)[b])
                q2[b, h] = (40.0 / D) * k[b, h, pi]
        if family == "pointer_onehot":
            hot = torch.zeros(L, dtype=torch.bool)
            hot[[r % L for r in ONEHOT_ROWS if r < L]] = True
            do = do * hot[None, None, :, None]
    else:
        raise ValueError(family)
    return (q2 / c2).to(BF16), k.to(BF16), v.to(BF16), do.to(BF16)


def make_decode_inputs(family, B, H, n, D, *, seed=0):
    """one pre-scaled query per (b, h) against n cache positions: q [B, H, 1, D], k / v [B, H, n, D] (bf16), the family's structure over the cache positions"""
    gen = torch.Generator().manual_seed(seed)
    q = 1.2 * torch.randn(B, H, 1, D, generator=gen) * (LOG2E / math.sqrt(D))
    k = 1.2 * torch.randn(B, H, n, D, generator=gen)
    v = 1.2 * torch.randn(B, H, n, D, generator=gen)
    j = torch.arange(n, dtype=torch.float32)
    if family == "ramp_up":            # the last split holds all the weight: the combine sees maxima that differ by hundreds
        q[..., D - 1], k[..., D - 1] = 1.0, 0.25 * j
    elif family == "ramp_down":
        q[..., D - 1], k[..., D - 1] = 1.0, 0.25 * (n - 1 - j)
    elif family == "spikes":
        k[:, :, spike_rows(n)] *= 6.0
    elif family == "pointer":
        k = torch.where(torch.rand(B, H, n, D, generator=gen) < 0.5, -1.0, 1.0)
        pi = torch.randint(0, n, (B, H), generator=gen)
        pi[0, 0], pi[-1, -1] = n - 1, 0      # the appended key, and the first one
        q = (40.0 / D) * torch.gather(k, 2, pi[:, :, None, None].expand(B, H, 1, D))
    else:
        raise ValueError(family)
    return q.to(BF16), k.to(BF16), v.to(BF16), (pi if family == "pointer" else None)


def doc_layouts(B, L):
    """the `contiguous` and `padding` packed-sample layouts of tests/test_gpu_kernels.py::_doc_layouts (same generator, same cuts)"""
    g = torch.Generator().manual_seed(L)
    sid = torch.zeros(B, L, dtype=torch.int64)
    cuts = sorted(torch.randint(1, L, (3,), generator=g).tolist())
    for i, c in enumerate(cuts):
        sid[:, c:] = i + 1
    sid[1 % B, -(L // 5 + 1):] = -1
    pad = sid.clone()
    pad[0] = -1
    pad[B - 1, L // 2:L // 2 + 70] = -1
    return dict(contiguous=sid, padding=pad)


# ------------------------------------------------------------------------------------------------ mask codes (class bits above the sample id)
def key_mask_codes(base, key_mask):
    """The engine's key-padding arithmetic (DIT._attention_masks, restated; tests/test_attention_mask_codes_ref64.py holds it to the product): on top of `base`
    codes (or zeros) a masked key gets key class 4, which no query mask contains; a key without a class becomes class 1, a query without a mask sees classes 1 | 2;
    the id field keeps its 32 bits (an id of -1 stays padding)."""
    base, km = torch.as_tensor(base).to(torch.int64), torch.as_tensor(key_mask).bool()
    kbits, qbits = (base >> 32) & 0xFF, (base >> 40) & 0xFF
    kbits = torch.where(km, torch.where(kbits == 0, 1, kbits), 4)
    qbits = torch.where(qbits == 0, 3, qbits)
    return ((base & 0xFFFFFFFF) | (kbits << 32) | (qbits << 40)).contiguous()


def key_mask_rows(L):
    """bool [4, L] (True = the key is attended): a few keys inside a tile; the whole first key tile; a stretch across two tile seams; every key"""
    assert L >= 200
    km = torch.ones(4, L, dtype=torch.bool)
    km[0, 5:9] = False
    km[1, 0:64] = False
    km[2, 130:200] = False
    km[3, :] = False
    return km


def code_layouts(B, L, Lt):
    """named [B, L] int64 mask-code layouts (B = 4): `modality` - the four (txt_drop, img_drop) combinations of the product's modality_mask_codes, text below Lt;
    `keypad` - sample 0 under key_mask_rows; `modality_keypad` - that key mask on the modality codes; `docs_keypad` - on the packed ids of
    doc_layouts(B, L)["contiguous"] (three cuts, one sample with trailing -1 padding); `docs_keypad_neg` - the same with the padding's id -2, which only the
    sign test of the predicate (id >= 0) reads as padding"""
    from unidisc_amd.kernels import modality_mask_codes

    assert B == 4
    modality = modality_mask_codes(torch.tensor([False, True, False, True]), torch.tensor([False, False, True, True]), Lt, L)
    km = key_mask_rows(L)
    docs = doc_layouts(B, L)["contiguous"]
    return dict(modality=modality, keypad=key_mask_codes(torch.zeros(B, L, dtype=torch.int64), km), modality_keypad=key_mask_codes(modality, km),
                docs_keypad=key_mask_codes(docs, km), docs_keypad_neg=key_mask_codes(torch.where(docs < 0, -2, docs), km))
