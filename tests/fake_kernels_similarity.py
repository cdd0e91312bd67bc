"""CPU stand-ins for the two likelihood-scoring kernels (`udm_subs_logp_rows`, `udm_likelihood_scores`) on top of tests/fake_kernels.py: everything that
module defines, plus these two.  Test doubles only - nothing in the product imports them, and the product has no CPU path."""
import torch

from fake_kernels import *  # noqa: F401,F403
from fake_kernels import _valid


def subs_logp_rows(logits, x0, modality, V, Vt, mask_id, restrict, logits_u=None, w=None):
    """log p(x0) of all-[MASK] rows: z = (1 + w) logits - w logits_u in fp32, log-sum-exp over the ids valid for the row, -1e6 for an invalid x0."""
    M = logits.shape[0]
    z = logits[:, :V].float()
    if logits_u is not None:
        z = (1.0 + w[:, None]) * z - w[:, None] * logits_u[:, :V].float()
    z = z.masked_fill(~_valid(M, V, Vt, mask_id, modality, restrict), float("-inf"))
    lse = torch.logsumexp(z, -1)
    zx = z.gather(1, x0[:, None])[:, 0]
    zx = torch.where(torch.isinf(zx), torch.full_like(zx, -1e6), zx)
    return zx - lse


def likelihood_scores(log_p, rows, w_std, valid_count, L):
    """(weighted, unweighed) [S]: per-sample sums of -log_p (x w_std) over the sample's segment of `rows`, divided by valid_count."""
    S = w_std.numel()
    seg = torch.div(rows, L, rounding_mode="floor")
    nl = -log_p.float()
    unweighed = torch.zeros(S, dtype=torch.float32).index_add_(0, seg, nl)
    weighted = torch.zeros(S, dtype=torch.float32).index_add_(0, seg, nl * w_std[seg])
    return weighted / valid_count, unweighed / valid_count
