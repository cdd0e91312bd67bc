"""CPU stand-ins for the key-split rectangular attention (K.attention_fwd_kv_split, K.attention_kv_split_plan, K.attention_kv_split_ws) on top of
tests/fake_kernels_kv.py: everything that module defines, plus the dense rectangular attention under the split entry point's signature - a split changes how the
work is spread, not what is computed, so the double ignores the workspace and the count.  The attention is written exactly as tests/fake_kernels.py::_attn
writes the square one (same operations in the same order on the same keys), so that a row of the rectangular call and the same row of an unmasked square call
go through the same arithmetic.  A test double only - nothing in the product imports it, and the product has no CPU path."""
import math

import torch

from fake_kernels_kv import *  # noqa: F401,F403
from fake_kernels_kv import attention_q_scale

CALLS = []      # (B, Lq, Lk, slots of the cache, ws is None) of every split call, for the tests that count them


def attention_kv_split_plan(B, Lq, Lk, H, D, splits=0):
    return 1, 0


def attention_kv_split_ws(B, Lq, Lk, H, D, device, splits=0):
    return None


def attention_fwd_kv_split(q, k_cache, v_cache, B, Lq, Lk, H, D, q_prescaled=False, out=None, want_lse=False, ws=None, splits=0):
    """q: a row view [B Lq, H D]; the caches [B', Lmax, H D] with B' >= B and Lmax >= Lk.  Slots >= Lk are never read."""
    CALLS.append((B, Lq, Lk, tuple(k_cache.shape), ws is None))
    qs = attention_q_scale(D) if q_prescaled else 1.0
    qh = (q.float() / qs).reshape(B, Lq, H, D).transpose(1, 2)
    kh = k_cache[:B, :Lk].float().reshape(B, Lk, H, D).transpose(1, 2)
    vh = v_cache[:B, :Lk].float().reshape(B, Lk, H, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    o = (p @ vh).transpose(1, 2).reshape(B * Lq, H * D).bfloat16()
    if out is not None:
        out.copy_(o)
        o = out
    if want_lse:
        return o, torch.logsumexp(s, -1) * 1.4426950408889634
    return o
