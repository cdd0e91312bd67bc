"""CPU stand-in for `udm_reveal_rows` (K.reveal_rows, K.reveal_supported) on top of tests/fake_kernels_cond.py and tests/fake_kernels_nucleus.py: everything those modules define, plus the
rules of csrc/reveal.hip through tests/reveal_ref.py (the kernel's Philox layout included).  A test double only - nothing in the product imports it, and the
product has no CPU path."""
import torch

import reveal_ref as R
from fake_kernels_cond import *  # noqa: F401,F403
from fake_kernels_nucleus import *  # noqa: F401,F403

REVEAL_CALLS = []   # one dict per call: what the sampler handed over (tests/test_reveal_host.py reads it)


def reveal_supported(x):
    return x.dim() == 2 and x.shape[1] <= 8192


def reveal_rows(x, mask_id, *, rows=None, tok=None, logp=None, sched=None, t=None, noise=None, out_noise=None, seed=0, r_temp=0.0, lottery=False, eos_id=None,
                pad_id=None, modality=None, x0=None, x0_unmask=None):
    B, L = x.shape
    REVEAL_CALLS.append(dict(n=0 if rows is None else int(rows.numel()), sched=sched, lottery=lottery, eos_id=eos_id, pad_id=pad_id, x0=x0 is not None,
                             noise=noise is not None, shape=(B, L)))
    if noise is None and sched is not None:
        words = R.philox_words(int(seed), B, L)
        noise = R.philox_uniform32(words) if lottery else R.philox_gumbel64(words).to(torch.float32)
    if out_noise is not None and noise is not None:
        out_noise.copy_(noise)
    return R.reveal_ref(x, mask_id, rows=rows, tok=tok, logp=logp, sched=sched, t=t, noise=noise, r_temp=r_temp, lottery=lottery, eos_id=eos_id, pad_id=pad_id,
                        modality=modality, x0=x0, x0_unmask=x0_unmask)
