"""CPU stand-in for `udm_attention_fwd_kv` (K.attention_fwd_kv) on top of tests/fake_kernels.py: everything that module defines, plus a dense rectangular
attention with the rounding points of its `_attn` (fp32 softmax, bf16 output).  A test double only - nothing in the product imports it, and the product
has no CPU path."""
import math

import torch

from fake_kernels import *  # noqa: F401,F403
from fake_kernels import attention_q_scale


def attention_fwd_kv(q, k_cache, v_cache, B, Lq, Lk, H, D, q_prescaled=False, out=None, want_lse=False):
    """q: a row view [B Lq, H D]; the caches [B', Lmax, H D] with B' >= B and Lmax >= Lk.  Slots >= Lk are never read."""
    qs = attention_q_scale(D) if q_prescaled else 1.0
    qh = (q.float() / qs).reshape(B, Lq, H, D).transpose(1, 2)
    kh = k_cache[:B, :Lk].float().reshape(B, Lk, H, D).transpose(1, 2)
    vh = v_cache[:B, :Lk].float().reshape(B, Lk, H, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * Lq, H * D).bfloat16()
    if out is not None:
        out.copy_(o)
        o = out
    if want_lse:
        return o, torch.logsumexp(s, -1) * 1.4426950408889634
    return o
