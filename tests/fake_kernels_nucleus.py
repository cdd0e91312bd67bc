"""CPU stand-ins for `udm_nucleus_sample_rows` / `udm_ar_nucleus_rows` (K.nucleus_sample_rows, K.ar_nucleus_rows, K.nucleus_supported) on top of
tests/fake_kernels.py: everything that module defines, plus the top-p rule of csrc/nucleus.hip in tensor operators (stable order, prefix with cumulative
p <= budget, the exponential race).  A test double only - nothing in the product imports it, and the product has no CPU path."""
import torch

from fake_kernels import *  # noqa: F401,F403


def nucleus_supported(logits, V):
    return True


def _draw(z, valid, inv_temperature, budget, u):
    """(token, log p_1(token), kept) per row: z fp32 [M, V], valid bool [M, V], u fp32 [M, V]"""
    M, V = z.shape
    p = torch.softmax((z.double() * inv_temperature).masked_fill(~valid, float("-inf")), -1)
    key = torch.where(valid, -p, torch.full_like(p, float("inf")))
    order = torch.sort(key, dim=-1, stable=True)[1]
    live = torch.arange(V)[None] < valid.sum(-1, keepdim=True)
    keep = ((p.gather(1, order).cumsum(-1) <= budget) & live).sum(-1).clamp(min=1)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(V)[None].expand(M, V))
    score = torch.where((rank < keep[:, None]) & valid, p / (1e-10 - torch.log((u + 1e-10).double())), torch.full_like(p, -1.0))
    tok = score.argmax(-1)
    logp = torch.log_softmax(z.double().masked_fill(~valid, float("-inf")), -1).gather(1, tok[:, None])[:, 0].float()
    return tok, logp, keep


def _valid(M, V, Vt, mask_id, modality, restrict):
    ids = torch.arange(V)[None]
    v = torch.ones(M, V, dtype=torch.bool)
    if restrict:
        v = torch.where((modality == 1)[:, None], ids >= Vt, ids < Vt).clone()
    v[:, mask_id] = False
    return v


def nucleus_sample_rows(logits, V, Vt, mask_id, *, inv_temperature, budget, modality=None, restrict=False, u=None, seed=0, logits_u=None, w=None,
                        want_keep=False):
    M = logits.shape[0]
    z = logits[:, :V].float()
    if logits_u is not None:
        z = (1 + w[:, None]) * z - w[:, None] * logits_u[:, :V].float()
    if u is None:
        u = torch.rand(M, V, generator=torch.Generator().manual_seed(int(seed) & 0x7FFFFFFF))
    tok, logp, keep = _draw(z, _valid(M, V, Vt, mask_id, modality, restrict), inv_temperature, budget, u[:, :V].float())
    return (tok, logp, keep) if want_keep else (tok, logp)


def ar_nucleus_rows(logits, x, pos, V, Vt, mask_id, *, inv_temperature, budget, step=0, modality=None, restrict=False, u=None, u_col0=0, seed=0, x0=None,
                    x0_unmask=None, next_ids=None, logits_u=None, w=None, rows=None):
    R = x.shape[0] if rows is None else rows
    z = logits[:R, :V].float()
    if logits_u is not None:
        z = (1 + w[0]) * z - w[0] * logits_u[:R, :V].float()
    if u is None:
        uu = torch.rand(R, V, generator=torch.Generator().manual_seed((int(seed) + 1000003 * (int(step) + 1)) & 0x7FFFFFFF))
    else:
        uu = u[:R, u_col0:u_col0 + V].float()
    tok, _, _ = _draw(z, _valid(R, V, Vt, mask_id, modality[:R, pos] if modality is not None else None, restrict), inv_temperature, budget, uu)
    keep = x0_unmask[:R, pos] if x0_unmask is not None else torch.zeros(R, dtype=torch.bool)
    val = torch.where(keep, x0[:R, pos], tok) if x0_unmask is not None else tok
    x[:R, pos] = val
    if next_ids is not None:
        next_ids[:R] = val
        if logits_u is not None:
            next_ids[R:2 * R] = torch.where(keep, torch.full_like(val, mask_id), val)
    return x
