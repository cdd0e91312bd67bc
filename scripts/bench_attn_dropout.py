"""Attention-probability dropout micro-bench: forward and backward wall time per call at p = 0 ON THE 8-WAVE KERNELS (generated programs switched off) and
at p = 0.1 (the same kernels with the mask), same inputs, alternating; the quantity of interest is time(p = 0.1) / time(p = 0).  One JSON line per case.
Per-kernel split of the backward (dQ | dK/dV): run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_attn_dropout.py` - the dropout
instantiations carry `AttnDrop` in their names."""
import json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unidisc_amd import kernels as K

def timeit(fn, n=20, w=5):
    for _ in range(w): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

# (name, B, H, L, D, causal): the 1.4 B headline shape, UniDisc-S, configs/experiments/jan_cub.yaml (txt 18 + img 128 on the `medium` preset), the AR baseline
CASES = [("1.4b", 8, 16, 1280, 128, False), ("unidisc-s", 64, 12, 384, 64, False), ("jan_cub", 16, 16, 146, 64, False), ("1.4b-causal", 8, 16, 1280, 128, True)]
P, REPS = 0.1, 5
for f in (K.set_attention_fwd64, K.set_attention_dq64, K.set_attention_dkv64):
    f(0)
for name, B, H, L, D, causal in CASES:
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, do = ((torch.randn(B * L, H * D, device="cuda", generator=g)).to(torch.bfloat16) for _ in range(4))
    kw = dict(q_prescaled=True, causal=causal)
    t = dict(fwd0=[], fwdp=[], bwd0=[], bwdp=[])
    for _ in range(REPS):   # alternate the two forms: drift of the box hits both
        for tag, dkw in (("0", {}), ("p", dict(dropout_p=P, seed=1234))):
            o, lse = K.attention_fwd_generic(q, k, v, B, L, H, D, **kw, **dkw)
            t["fwd" + tag].append(timeit(lambda: K.attention_fwd_generic(q, k, v, B, L, H, D, **kw, **dkw)))
            t["bwd" + tag].append(timeit(lambda: K.attention_bwd_generic(q, k, v, o, do, lse, B, L, H, D, **kw, **dkw)))
    m = {k_: statistics.median(v_) for k_, v_ in t.items()}
    spread = {k_: (max(v_) - min(v_)) / statistics.median(v_) for k_, v_ in t.items()}
    print(json.dumps(dict(case=name, B=B, H=H, L=L, D=D, causal=causal, p=P, fwd_ms_p0=round(m["fwd0"], 4), fwd_ms_p=round(m["fwdp"], 4),
                          fwd_ratio=round(m["fwdp"] / m["fwd0"], 3), bwd_ms_p0=round(m["bwd0"], 4), bwd_ms_p=round(m["bwdp"], 4),
                          bwd_ratio=round(m["bwdp"] / m["bwd0"], 3), max_rel_spread=round(max(spread.values()), 3))), flush=True)
