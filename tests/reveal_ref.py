"""The rules of `udm_reveal_rows` (include/unidisc_hip.h) as plain, exact torch statements on the CPU: the second half of a maskgit /
first_hitting sampler step (model_eval.py:3046-3114, :3005-3043), the padding behind the first EOS (:2390-2394) and the conditioning write-back (:2399).

    k_b          min(sched[b], number of [MASK] positions of row b); k_b <= 0 reveals nothing
    confidence   conf = logp + (fp32(r_temp) * g) * t_b: three fp32 tensor operations, each rounded once, defined on the [MASK] positions only (a [MASK]
                 position without an entry in `rows` has log p = -inf and its token stays [MASK]); thr = the k_b-th largest; every [MASK] position with
                 conf >= thr is revealed
    lottery      the first k_b [MASK] positions of the stable descending sort of the values: (value descending, position ascending)
    EOS rule     first = the smallest l of the whole row with x_new[l] == eos; l > first, modality 0, token neither pad nor [MASK] -> pad
    write-back   x_new = where(x0_unmask, x0, x_new), after the padding

`mutant=` seeds one wrong rule (MUTANTS); tests/test_reveal_ref.py shows that the comparison used everywhere (torch.equal on x_out) tells each from the rule.
The Philox layout of the kernel's own noise is restated in `philox_words` / `philox_uniform32` / `philox_gumbel64`."""
import numpy as np
import torch

from attn_prob_dropout_ref import philox4x32

F32 = torch.float32
MUTANTS = ("k_plus_one", "k_minus_one", "strict_gt", "k_unclamped", "conf_fma", "conf_order", "ties_desc_position", "pad_eos_itself", "pad_image", "pad_mask",
           "writeback_first", "first_eos_text_only")


def confidence(logp_full, g, t, r_temp, mutant=None):
    """[B, L] fp32: logp + (r_temp * g) * t with every operation rounded to fp32 (what `_maskgit_reveal` computes with tensor operators)"""
    r = torch.tensor(float(r_temp), dtype=F32)
    t_col = t.reshape(-1, 1).to(F32)
    if mutant == "conf_fma":       # one rounding for the last product and the sum
        return (logp_full.double() + (r * g.to(F32)).double() * t_col.double()).to(F32)
    if mutant == "conf_order":     # r_temp * (g * t)
        return logp_full + r * (g.to(F32) * t_col)
    return logp_full + (r * g.to(F32)) * t_col


def reveal_ref(x, mask_id, *, rows=None, tok=None, logp=None, sched=None, t=None, noise=None, r_temp=0.0, lottery=False, eos_id=None, pad_id=None,
               modality=None, x0=None, x0_unmask=None, mutant=None):
    """x_out int64 [B, L]; operands as unidisc_amd.kernels.reveal_rows, the noise always explicit"""
    assert mutant is None or mutant in MUTANTS, mutant
    B, L = x.shape
    m = x == mask_id
    pos = torch.arange(L)[None]
    pred = x.clone()
    lp = torch.full((B * L,), float("-inf"), dtype=F32)
    if rows is not None and rows.numel():
        pred.view(-1)[rows] = tok
        if logp is not None:
            lp[rows] = logp.to(F32)
    pred = torch.where(m, pred, x)
    reveal = torch.zeros_like(m)
    if sched is not None:
        k = sched.to(torch.int64)
        if mutant != "k_unclamped":
            k = torch.minimum(k, m.sum(-1))
        k = k + (1 if mutant == "k_plus_one" else 0) - (1 if mutant == "k_minus_one" else 0)
        if mutant in ("k_plus_one", "k_minus_one"):
            k = torch.minimum(k, m.sum(-1))
        v = noise.to(F32) if lottery else confidence(lp.view(B, L), noise, t, r_temp, mutant)
        v = torch.where(m, v, torch.full_like(v, float("-inf")))
        for b in range(B):
            kb = int(k[b])
            if kb <= 0:
                continue
            if lottery:
                if mutant == "ties_desc_position":
                    order = (L - 1) - torch.sort(v[b].flip(0), descending=True, stable=True)[1]
                else:
                    order = torch.sort(v[b], descending=True, stable=True)[1]
                reveal[b, order[:kb]] = True
                reveal[b] &= m[b]
            else:
                thr = torch.sort(v[b], descending=True)[0][kb - 1]      # (an unclamped k past L is an IndexError)
                reveal[b] = m[b] & ((v[b] > thr) if mutant == "strict_gt" else (v[b] >= thr))
    out = torch.where(reveal, pred, x)
    if mutant == "writeback_first" and x0 is not None:      # (and not behind the padding)
        out = torch.where(x0_unmask, x0, out)
    if eos_id is not None:
        is_eos = out == eos_id
        if mutant == "first_eos_text_only":
            is_eos = is_eos & (modality == 0)
        first = torch.where(is_eos.any(-1), is_eos.int().argmax(-1), torch.full((B,), L))[:, None]
        behind = (pos >= first) if mutant == "pad_eos_itself" else (pos > first)
        to_pad = behind & (out != pad_id)
        if mutant != "pad_image":
            to_pad = to_pad & (modality == 0)
        if mutant != "pad_mask":
            to_pad = to_pad & (out != mask_id)
        out = torch.where(to_pad, torch.full_like(out, pad_id), out)
    if x0 is not None and mutant != "writeback_first":
        out = torch.where(x0_unmask, x0, out)
    return out


# ------------------------------------------------------------------------------------------------ the kernel's own noise (noise = NULL)
def philox_words(seed, B, L):
    """int64 [B, L]: word >> 8 of Philox4x32-10 with key = seed, counter = b ceil(L / 4) + (l >> 2), word l & 3"""
    l = np.arange(L, dtype=np.uint64)[None]
    ctr = np.arange(B, dtype=np.uint64)[:, None] * np.uint64((L + 3) // 4) + (l >> np.uint64(2))
    w = np.stack(philox4x32(int(seed) & (2 ** 64 - 1), ctr), -1)
    w = np.take_along_axis(w, np.broadcast_to(l & np.uint64(3), ctr.shape)[..., None].astype(np.int64), -1)[..., 0]
    return torch.from_numpy((w >> np.uint64(8)).astype(np.int64))


def philox_uniform32(words):
    """the lottery value of a grid point x = word >> 8: fp32(fp32(x) + 0.5) 2^-24, capped at 1 - 2^-24 (the top of the grid would round to 1)"""
    u = (words.to(F32) + torch.tensor(0.5, dtype=F32)) * torch.tensor(2.0 ** -24, dtype=F32)
    return torch.minimum(u, torch.tensor(1.0 - 2.0 ** -24, dtype=F32))


def philox_gumbel64(words):
    """fp64 Gumbel noise of the exact grid point u = (x + 0.5) 2^-24"""
    return -torch.log(-torch.log((words.double() + 0.5) * 2.0 ** -24))


# ------------------------------------------------------------------------------------------------ cases (shared by the CPU and the GPU tests)
V, MASK, EOS, PAD, R_TEMP = 64, 40, 2, 0, 10.0       # plain tokens are drawn from 3 .. 39
SELECT_FAMILIES = ("random", "no_mask", "gap", "all_masked", "k0", "k1", "k_count", "k_above", "all_equal", "dup_cut", "neg_inf", "neg_inf_all", "t_one", "t_small",
                   "k_past_L", "fma_tie", "order_tie")
EOS_FAMILIES = ("eos_absent", "eos_at_0", "eos_last_text", "eos_revealed", "eos_several", "eos_in_x0", "eos_in_image")


def make_case(B, L, lottery, family="random", eos_family=None, with_x0=False, seed=0):
    """operands of reveal_ref / K.reveal_rows (CPU tensors) for one family of the selection and, optionally, one of the EOS rule.  Text is the first
    ceil(L / 2) positions (`eos_in_image`: the last ones, so that an EOS id at an image position comes first in the row)."""
    names = SELECT_FAMILIES + EOS_FAMILIES
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * names.index(family) + 131 * (names.index(eos_family) if eos_family else 0) + 17 * L + B + (5 if lottery else 0))
    rnd = lambda *s: torch.rand(*s, generator=g)
    Lt = (L + 1) // 2
    modality = torch.zeros(B, L, dtype=torch.int64)
    if eos_family == "eos_in_image":
        modality[:, : L - Lt] = 1
    else:
        modality[:, Lt:] = 1
    x = torch.randint(3, 40, (B, L), generator=g)
    masked = rnd(B, L) < 0.6
    if family == "no_mask":
        masked[:] = False
    elif family == "gap" and B >= 3:
        masked[1] = False
        masked[0, 0] = masked[2, L - 1] = True
    elif family == "all_masked":
        masked[:] = True
    x0 = x0_unmask = None
    if with_x0 or eos_family == "eos_in_x0":
        x0 = torch.randint(3, 40, (B, L), generator=g)
        x0_unmask = rnd(B, L) < 0.3
        if eos_family == "eos_in_x0":                 # given text: an EOS with given tokens behind it, which the write-back must restore
            x0_unmask[:, :Lt] = True
            x0[:, Lt // 2] = EOS
        x = torch.where(x0_unmask, x0, x)
        masked = masked & ~x0_unmask
    x = torch.where(masked, torch.full_like(x, MASK), x)
    text = (modality == 0).nonzero()
    if eos_family == "eos_at_0":
        x[:, 0] = EOS
    elif eos_family == "eos_last_text":
        x[:, Lt - 1] = EOS
    elif eos_family == "eos_several":
        x[rnd(B, L) < 0.2] = EOS
    elif eos_family == "eos_in_image":
        x[:, 0] = EOS                                 # an image position when L > 1; the text lies behind it
        if L - Lt > 1:
            x[:, L - Lt - 1] = 17
    if x0 is not None:
        x0 = torch.where(x0_unmask, x, x0)            # the conditioning is what the state holds at the given positions
    rows = (x.reshape(-1) == MASK).nonzero().reshape(-1)
    n = rows.numel()
    n_mask = (x == MASK).sum(-1)
    tok = torch.randint(3, 40, (n,), generator=g)
    logp = (-5 * rnd(n)).to(F32)
    t = (0.05 + 0.9 * rnd(B)).to(F32)
    noise = rnd(B, L).to(F32) if lottery else (-torch.log(-torch.log(rnd(B, L).double().clamp(1e-9, 1 - 1e-9)))).to(F32)
    sched = (rnd(B) * (n_mask + 1).float()).floor().to(torch.int64)
    if family == "k0":
        sched = torch.zeros(B, dtype=torch.int64)
    elif family == "k1":
        sched = torch.ones(B, dtype=torch.int64)
    elif family == "k_count":
        sched = n_mask.clone()
    elif family == "k_above":
        sched = n_mask + 3
    elif family == "all_equal":
        logp, noise = torch.full((n,), -1.0, dtype=F32), torch.full((B, L), 0.5, dtype=F32)
        sched = torch.clamp(n_mask // 2, min=1)
    elif family == "dup_cut":                         # a few distinct values: equal values straddle the cut
        logp, noise = torch.full((n,), -1.0, dtype=F32), (torch.randint(0, 4, (B, L), generator=g).float() / 4).to(F32)
        sched = torch.clamp(n_mask // 2, min=1)
    elif family in ("neg_inf", "neg_inf_all"):
        logp[rnd(n) < (0.5 if family == "neg_inf" else 2.0)] = float("-inf")
        sched = n_mask.clone() if family == "neg_inf" else torch.clamp(n_mask // 2, min=1)
    elif family == "t_one":
        t = torch.ones(B, dtype=F32)
    elif family == "t_small":
        t = torch.full((B,), 1e-5, dtype=F32)
    elif family == "k_past_L":
        sched = torch.full((B,), L + 5, dtype=torch.int64)
    elif family in ("fma_tie", "order_tie") and not lottery:
        # two [MASK] positions per sample whose confidences are EQUAL under the three rounded operations and differ when the last two are fused (fma_tie) or
        # the products are taken in the other order (order_tie): k = 1 reveals both, a kernel that rounds differently reveals one
        logp, noise = torch.full((n,), -60.0, dtype=F32), torch.zeros(B, L, dtype=F32)
        sched = torch.ones(B, dtype=torch.int64)
        wrong = "conf_fma" if family == "fma_tie" else "conf_order"
        for b in range(B):
            mine = ((rows >= b * L) & (rows < (b + 1) * L)).nonzero().reshape(-1)
            if mine.numel() < 2:
                continue
            ja, jb = int(mine[0]), int(mine[-1])
            for _ in range(10000):
                lp_a, g_a = (-3 * rnd(1)).to(F32), (4 * rnd(1) - 1).to(F32)
                right = confidence(lp_a, g_a, t[b:b + 1], R_TEMP)
                if not torch.equal(right, confidence(lp_a, g_a, t[b:b + 1], R_TEMP, wrong)):
                    break
            else:
                raise AssertionError("no rounding difference found")
            logp[ja], noise.view(-1)[rows[ja]] = lp_a[0], g_a[0]
            logp[jb] = right.reshape(-1)[0]                  # + (r_temp * 0) * t: exact in every form
    if eos_family == "eos_revealed" and n > 0:        # an EOS is drawn at a text [MASK] position and wins the step
        flat_text = (modality.reshape(-1)[rows] == 0).nonzero().reshape(-1)
        for j in flat_text[:: max(1, flat_text.numel() // (2 * B))].tolist():
            tok[j] = EOS
            logp[j] = 0.0
            noise.view(-1)[rows[j]] = 2.0 if lottery else 30.0
        sched = torch.clamp(sched, min=1)
    case = dict(x=x, rows=rows, tok=tok, logp=None if lottery else logp, sched=sched, t=None if lottery else t, noise=noise, r_temp=0.0 if lottery else R_TEMP,
                lottery=lottery, modality=modality if eos_family else None, eos_id=EOS if eos_family else None, pad_id=PAD if eos_family else None, x0=x0,
                x0_unmask=x0_unmask)
    return case


def all_cases(B, L, lottery, seed=0):
    """{name: case}: every selection family without the EOS rule, with and without x0; every EOS family on the random selection, with and without x0"""
    out = {}
    for f in SELECT_FAMILIES:
        for w in (False, True):
            out[f"{f}{'+x0' if w else ''}"] = make_case(B, L, lottery, f, None, w, seed)
    for e in EOS_FAMILIES:
        for w in (False, True):
            out[f"{e}{'+x0' if w else ''}"] = make_case(B, L, lottery, "random", e, w, seed)
        out[f"{e}+k0"] = make_case(B, L, lottery, "k0", e, False, seed)
    return out
