"""Shared by tests/test_modality_cache_host.py (CPU, kernel doubles) and tests/test_gpu_modality_cache.py: the `c_large` product with
eval.attention_caching (and the extension key eval.attention_caching_read_cache), and the comparison of masked-row logits between a text-slice forward and
the text rows of a full-length forward."""
import torch

from golden_utils import Golden
from product_utils import build_product

# a read-cache text step against the text rows of the masked full-length forward, relative L2 error per logits row: the bound tests/test_gpu_ar_sampler.py
# holds KV-cached decode rows to against the full causal forward (two bf16 evaluation orders of the same function)
ROW_BOUND = 1e-2


def load_caching_golden():
    from test_sampler import load_sampler
    return Golden("c_large"), load_sampler("c_large_attn_caching")


def caching_product(device, read_cache):
    """read_cache: True / False, or None for the key left out"""
    from unidisc_amd.config import Cfg

    g, s = load_caching_golden()
    diff = build_product(g, device=device)
    diff.backbone.eval()
    kw = {} if read_cache is None else dict(attention_caching_read_cache=bool(read_cache))
    diff.config.eval = Cfg(cfg=None, attention_caching=True, attention_caching_txt_to_img_ratio=int(s["ratio"]), **kw)
    return g, s, diff


def build_mask(B, Lt, device):
    from unidisc_amd.dit import ModalityMask
    return ModalityMask(torch.zeros(B, dtype=torch.bool, device=device), torch.ones(B, dtype=torch.bool, device=device), Lt)


def text_rows_of_full(out, L, Lt, V):
    """(logits, rows, n) of a [B, L] forward -> (fp32 logits [n_text, V] of the [MASK] rows at positions < Lt, their indices b Lt + l), sorted by index"""
    logits, rows, n = out[:3]
    r = rows[:n]
    keep = (r % L) < Lt
    key = torch.div(r[keep], L, rounding_mode="floor") * Lt + r[keep] % L
    order = torch.argsort(key)
    return logits[:n][keep][order][:, :V].float(), key[order]


def text_rows(out, V):
    """(logits, rows, n) of a [B, Lt] forward, sorted by row index"""
    logits, rows, n = out[:3]
    order = torch.argsort(rows[:n])
    return logits[:n][order][:, :V].float(), rows[:n][order]


def worst_row_rel_err(got, ref):
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())
