"""The AR baseline's training step (parameterization=ar, trainer.ar_shift, model.full_attention=false: configs/experiments/ar.yaml) at the two
workloads of bench.py - UniDisc-S (B = 64, L = 384) and 1.4 B (B = 8, L = 1280) - beside the SUBS step of the same model, and the per-layer time of the
causal attention kernels against the bidirectional ones at the same shape (engine layout, q pre-scaled, forward + backward of one block).

    python scripts/bench_ar_step.py [--steps 10] [--warmup 3] [--attn-only]

Prints one JSON line.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_ar_step.py --attn-only`: the
causal calls run the 8-wave kernels of csrc/attention.hip (attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel with CAUSAL = true), the
bidirectional ones whatever the dispatch picks at that shape (at head dim 128 the generated one-wave-per-SIMD programs)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from unidisc_amd import kernels as K  # noqa: E402

WORKLOADS = {"unidisc-s-l384": 64, "unidisc-1.4b-l1280": 8}


def step_ms(diff, batch, steps, warmup):
    for i in range(warmup):
        diff.training_step(batch, i).loss.backward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = diff.training_step(batch, warmup + i)
        out.loss.backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(out.loss.detach())


def attn_ms(B, L, H, D, causal, reps, dev):
    """forward + backward of one block's attention in the engine's layout (q | k in [M, 2d], v at column 2d of [M, 3d]), q pre-scaled"""
    d, M = H * D, B * L
    g = torch.Generator(device=dev).manual_seed(1)
    qkr = (torch.randn(M, 2 * d, device=dev, generator=g) * torch.cat([torch.full((d,), K.attention_q_scale(D)), torch.ones(d)]).to(dev)).bfloat16()
    qkv = torch.randn(M, 3 * d, device=dev, generator=g).bfloat16()
    do = torch.randn(M, d, device=dev, generator=g).bfloat16()
    dqkr, dqkv = torch.empty_like(qkr), torch.empty_like(qkv)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fwd = bwd = 0.0
    for i in range(reps + 2):
        ev[0].record()
        o, lse = K.attention_fwd(qkr, qkv, B, L, H, D, q_prescaled=True, causal=causal)
        ev[1].record()
        K.attention_bwd(qkr, qkv, o, do, lse, dqkr, dqkv, B, L, H, D, q_prescaled=True, causal=causal)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 2:
            fwd += ev[0].elapsed_time(ev[1]) / reps
            bwd += ev[1].elapsed_time(ev[2]) / reps
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--attn-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    for wl, B in WORKLOADS.items():
        w = bench.WORKLOADS[wl]
        L = w["txt_length"] + w["img_length"]
        r = dict(B=B, L=L)
        if not args.attn_only:
            batch = {k: v.to(dev) for k, v in bench.synthetic_batch(wl, B, 42).items()}
            for mode in ("subs", "ar"):
                torch.manual_seed(42)
                cfg, diff = bench.build(wl, dev, 0.1)
                if mode == "ar":
                    del diff
                    from unidisc_amd import Diffusion

                    cfg.parameterization, cfg.trainer.ar_shift, cfg.model.full_attention = "ar", True, False
                    diff = Diffusion(cfg, None, dev)
                    diff.backbone.train()
                ms, loss = step_ms(diff, batch, args.steps, args.warmup)
                r[f"{mode}_step_ms"], r[f"{mode}_loss"] = round(ms, 2), round(loss, 4)
                r[f"{mode}_tokens_per_s"] = round(B * L / ms * 1e3)
                del diff, cfg
                torch.cuda.empty_cache()
        from unidisc_amd import MODEL_PRESETS

        p = MODEL_PRESETS[w["preset"]]
        H, D = p["n_heads"], p["hidden_size"] // p["n_heads"]
        for causal in (False, True):
            f, b = attn_ms(B, L, H, D, causal, 10, dev)
            tag = "causal" if causal else "bidir"
            r[f"attn_{tag}_fwd_ms"], r[f"attn_{tag}_bwd_ms"] = round(f, 4), round(b, 4)
        r["attn_causal_over_bidir"] = round((r["attn_causal_fwd_ms"] + r["attn_causal_bwd_ms"]) / (r["attn_bidir_fwd_ms"] + r["attn_bidir_bwd_ms"]), 3)
        r.update(H=H, D=D)
        res[wl] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
