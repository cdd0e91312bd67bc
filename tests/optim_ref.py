"""float64 reference of one optimizer step as csrc/optim.hip defines it: `clip_grad_norm_`, torch's AdamW (decoupled decay, single-tensor
form) and the parameter EMA of the reference's models/ema.py, written from the definitions - not from the kernels or their CPU doubles
(this module imports neither).

    clip = min(1, max_norm / (sqrt(sum g^2) + 1e-6))        (no clipping: 1)
    g    = g * clip
    p    = p * (1 - lr * wd)                                (decay BEFORE the update)
    m    = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g g
    p    = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)     (eps AFTER the bias-corrected square root)
    ema  = ema - (1 - decay) (ema - p)                      (from the UPDATED parameter)
"""
import math

import torch

F64 = torch.float64


def sumsq64(grads):
    """sum of squares of every element of every gradient, accumulated in float64 (python float)"""
    return float(sum((g.detach().to("cpu", F64) ** 2).sum() for g in grads))


def clip_coef64(gsq, max_norm):
    if max_norm is None:
        return 1.0
    return min(1.0, float(max_norm) / (math.sqrt(gsq) + 1e-6))


def ema_decay_at(decay, n):
    """decay of the n-th EMA update (n = 1, 2, ...) with the warm-up of models/ema.py:46-49"""
    return min(decay, (1 + n) / (10 + n))


def adamw_step64(p, g, m, v, ema, *, lr, betas, eps, weight_decay, step, gsq=None, max_norm=None, ema_decay=0.0):
    """One step.  p, g, m, v, ema (or None): the fp32 tensors the kernel got (any device); gsq: sum of squares of ALL gradients of the step in float64 (needed when
    max_norm is given).  Returns new (p, m, v, ema) as float64 CPU tensors; the inputs are not modified."""
    p, g, m, v = (t.detach().to("cpu", F64) for t in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    g = g * clip_coef64(gsq, max_norm)
    p = p * (1.0 - float(lr) * float(weight_decay))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    p = p - (float(lr) / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + float(eps)))
    e = None
    if ema is not None:
        e = ema.detach().to("cpu", F64)
        e = e - (1.0 - float(ema_decay)) * (e - p)
    return p, m, v, e
