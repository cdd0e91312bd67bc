"""Attention-probability dropout (model.attn_dropout): the keep mask of include/unidisc_hip.h restated in numpy from the header's text, and dense fp32
attention with that mask - the reference of tests/test_attention_prob_dropout.py (CPU) and tests/test_gpu_attention_prob_dropout.py.

    thr   = (uint32)(p * 65536 + 0.5)                                          (fp32 arithmetic)
    ctr   = ((b * H + h) * ceil(L / 2) + (i >> 1)) * ceil(L / 4) + (j >> 2)      one Philox4x32-10 call per patch of 2 queries x 4 keys
    field = 16-bit lane (i & 1) * 4 + (j & 3) of philox4x32(seed, ctr), lanes in the order x.lo x.hi y.lo y.hi z.lo z.hi w.lo w.hi
    Z[b, h, i, j] = field >= thr;   O = (Z o softmax(S)) V / (1 - p)
"""
import math

import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(seed, ctr):
    """Philox4x32-10 as csrc/common.h runs it: key = the two halves of `seed`, counter = (ctr.lo, ctr.hi, 0x5bd1e995, 0x27d4eb2f)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2, c3 = np.full_like(c0, 0x5BD1E995), np.full_like(c0, 0x27D4EB2F)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def threshold(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_mask(seed, p, B, H, L):
    """bool [B, H, L, L] numpy: True = kept."""
    thr = threshold(p)
    R2, G4 = (L + 1) // 2, (L + 3) // 4
    row = np.arange(B * H * R2, dtype=np.uint64)[:, None]                    # (b * H + h) * R2 + (i >> 1)
    ctr = row * np.uint64(G4) + np.arange(G4, dtype=np.uint64)[None]         # [B H R2, G4]
    w = philox4x32(seed, ctr)
    f = np.stack([x for wd in w for x in (wd & np.uint64(0xFFFF), wd >> np.uint64(16))], -1)   # [B H R2, G4, 8]: lane = (i & 1) * 4 + (j & 3)
    f = f.reshape(B, H, R2, G4, 2, 4).transpose(0, 1, 2, 4, 3, 5).reshape(B, H, R2 * 2, G4 * 4)
    return (f >= thr)[:, :, :L, :L]


def dense_attention(q, k, v, B, L, H, D, keep=None, p=0.0, causal=False):
    """q, k, v fp32 [B * L, H * D] -> [B * L, H * D]: softmax(q k^T / sqrt(D)) o keep / (1 - p) @ v, differentiable.  keep: bool [B, H, L, L] or None."""
    q, k, v = (t.reshape(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * torch.as_tensor(keep).to(pr.dtype) * (1.0 / (1.0 - float(np.float32(p))))
    return (pr @ v).transpose(1, 2).reshape(B * L, H * D)
