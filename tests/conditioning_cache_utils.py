"""Shared by tests/test_conditioning_cache_host.py (CPU, kernel doubles) and tests/test_gpu_conditioning_cache.py: the `c_large` product (d = 64, H = 2, D = 32,
L = 16 + 16, 2-D rope, modality embedding) with the extension key eval.conditioning_cache, conditioning inputs with one modality fully given, and the reference
every comparison is made against - the full-length forward under the ModalityMask that blinds the given modality's queries to the other modality."""
import torch

from golden_utils import Golden
from product_utils import build_product

PREDICTORS = ("ddpm_cache", "maskgit", "maskgit_nucleus", "first_hitting")


def cond_product(device, key=True, cfg=None, split=False, **extra):
    """key: True / False, or None for the key left out"""
    from unidisc_amd.config import Cfg

    g = Golden("c_large")
    diff = build_product(g, device=device)
    diff.backbone.eval()
    kw = {} if key is None else dict(conditioning_cache=bool(key))
    diff.config.eval = Cfg(cfg=cfg, split_cfg_batches=bool(split), **kw, **extra)
    return g, diff


def conditioning(g, diff, B, given, inpaint=False, seed=0, device="cpu"):
    """x0, x0_unmask, modality [B, L]: the `given` modality ("text" / "image") fully given, the other all [MASK] - or, with `inpaint`, partly given too"""
    Lt, Li = g.case["txt_length"], g.case["img_length"]
    Vt, V = g.case["text_vocab_size"], g.case["vocab_size"]
    gen = torch.Generator().manual_seed(1000 + seed)
    x0 = torch.cat([torch.randint(0, diff.mask_index, (B, Lt), generator=gen), torch.randint(Vt, V, (B, Li), generator=gen)], 1)
    unmask = torch.zeros(B, Lt + Li, dtype=torch.bool)
    gsl, osl = (slice(0, Lt), slice(Lt, Lt + Li)) if given == "text" else (slice(Lt, Lt + Li), slice(0, Lt))
    unmask[:, gsl] = True
    if inpaint:
        unmask[:, osl] = torch.rand(B, osl.stop - osl.start, generator=gen) < 0.3
    modality = torch.cat([torch.zeros(B, Lt, dtype=torch.int64), torch.ones(B, Li, dtype=torch.int64)], 1)
    return x0.to(device), unmask.to(device), modality.to(device), osl


def build_mask(rows, Lt, given, device):
    """text given: text queries see text keys only (txt_drop = 1); image given: image queries see image keys only (img_drop = 1)"""
    from unidisc_amd.dit import ModalityMask
    on, off = torch.ones(rows, dtype=torch.bool, device=device), torch.zeros(rows, dtype=torch.bool, device=device)
    return ModalityMask(on if given == "text" else off, on if given == "image" else off, Lt)


def slice_rows_of_full(out, L, sl, V):
    """(logits, rows, n) of a [R, L] forward -> (fp32 logits of its [MASK] rows inside positions sl, their indices r len(sl) + l - sl.start), in the forward's order"""
    logits, rows, n = out[:3]
    r = rows[:n]
    keep = ((r % L) >= sl.start) & ((r % L) < sl.stop)
    key = torch.div(r[keep], L, rounding_mode="floor") * (sl.stop - sl.start) + r[keep] % L - sl.start
    return logits[:n][keep][:, :V].float(), key


def slice_rows(out, V):
    logits, rows, n = out[:3]
    return logits[:n][:, :V].float(), rows[:n]


def worst_row_rel_err(got, ref):
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())


def reference_backbone(diff, g, given, x_given, B):
    """Replaces diff.backbone.forward_masked_logits by the reference the conditioning cache is held to: every call - "build" or "read" - becomes the full-length
    forward under the build mask, without any cache; a "read" call's generated slice is put behind / in front of the given tokens (`x_given` [B, given length];
    all [MASK] in the unconditional rows [B, 2 B) of guided sampling) and the rows of the answer are re-indexed for the slice.  Returns the list of calls."""
    bb = diff.backbone
    fwd = bb.forward_masked_logits
    Lt, L = g.case["txt_length"], g.case["txt_length"] + g.case["img_length"]
    sl = slice(Lt, L) if given == "text" else slice(0, Lt)
    Lq = sl.stop - sl.start
    calls, state = [], dict(mod=None)

    def join(given_part, gen_part):
        return torch.cat([given_part, gen_part], 1) if given == "text" else torch.cat([gen_part, given_part], 1)

    def ref_fwd(xt, sigma=None, modality=None, plan_ids=None, conditioning_cache=None, cache_row0=0, **kw):
        assert conditioning_cache in ("build", "read") and not kw, (conditioning_cache, kw)
        rows = xt.shape[0]
        calls.append((conditioning_cache, tuple(xt.shape), cache_row0, plan_ids is not None))
        mask = build_mask(rows, Lt, given, xt.device)
        if conditioning_cache == "build":
            state["mod"] = modality[:B] if modality is not None else None
            return fwd(xt, sigma, modality=modality, plan_ids=plan_ids, block_mask=mask)
        halves = [(cache_row0 + r) // B for r in range(rows)]
        giv = torch.stack([x_given[(cache_row0 + r) % B] if h == 0 else torch.full_like(x_given[0], diff.mask_index) for r, h in enumerate(halves)])
        full = join(giv, xt)
        plan = None if plan_ids is None else join(torch.stack([x_given[(cache_row0 + r) % B] for r in range(rows)]), plan_ids)      # no [MASK] in the given part
        mod = None if state["mod"] is None else torch.cat([state["mod"]] * (rows // B), 0)
        logits, frows, n = fwd(full, sigma, modality=mod, plan_ids=plan, block_mask=mask)
        pos = frows % L
        assert bool(((pos[:n] >= sl.start) & (pos[:n] < sl.stop)).all())
        srows = torch.div(frows, L, rounding_mode="floor") * Lq + (pos - sl.start).clamp(0, Lq - 1)
        return logits, srows, n

    bb.forward_masked_logits = ref_fwd
    return calls
