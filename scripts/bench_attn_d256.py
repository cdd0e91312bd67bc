"""Attention at head dim 256 (the xxl model: d = 4096, H = 16): forward + backward of one block's attention in the engine's layout (q | k in [M, 2d], v at column
2d of [M, 3d]), q pre-scaled, timed with events - bidirectional and causal at (B, H, L, D) = (8, 16, 1280, 256) - beside the SAME build's head-dim-128 kernels
at (8, 32, 1280, 128): equal flops and equal operand bytes.  The yardstick is the 8-wave kernels of csrc/attention.hip (generated programs switched off; the
same shape with them on is printed for information).  Reported: time(D = 256) / time(D = 128, 8-wave), forward and backward separately; medians of `--reps`
timing rounds of `--iters` calls each, the shapes alternating inside a round.

    python scripts/bench_attn_d256.py [--reps 11] [--iters 10]      one JSON line (kernel level)
    python scripts/bench_attn_d256.py --step [--steps 10] [--warmup 3] [--batch 4] [--blocks 30]
        one training step of MODEL_PRESETS["xxl"] (fwd + bwd, dropout 0.1, L = 1280): ms_per_step, tokens/s, peak memory, MFU with bench.py's F_tok

Per-kernel split: `rocprofv3 --kernel-trace --stats -- python scripts/bench_attn_d256.py` (the D = 256 backward is attn_bwd_dq_kernel plus two
attn_bwd_dkv_kernel launches, MODE 1 = dK and MODE 2 = dV)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from unidisc_amd import kernels as K  # noqa: E402

L_SEQ, TXT, IMG = 1280, 256, 1024


class AttnCase:
    def __init__(self, B, H, L, D, causal, dev):
        self.B, self.H, self.L, self.D, self.causal = B, H, L, D, causal
        d, M = H * D, B * L
        g = torch.Generator(device=dev).manual_seed(1)
        self.qkr = (torch.randn(M, 2 * d, device=dev, generator=g) * torch.cat([torch.full((d,), K.attention_q_scale(D)), torch.ones(d)]).to(dev)).bfloat16()
        self.qkv = torch.randn(M, 3 * d, device=dev, generator=g).bfloat16()
        self.do = torch.randn(M, d, device=dev, generator=g).bfloat16()
        self.dqkr, self.dqkv = torch.empty_like(self.qkr), torch.empty_like(self.qkv)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def round(self, iters):
        """(fwd ms, bwd ms) per call over `iters` calls"""
        kw = dict(q_prescaled=True, causal=self.causal)
        o, lse = K.attention_fwd(self.qkr, self.qkv, self.B, self.L, self.H, self.D, **kw)
        self.ev[0].record()
        for _ in range(iters):
            o, lse = K.attention_fwd(self.qkr, self.qkv, self.B, self.L, self.H, self.D, **kw)
        self.ev[1].record()
        for _ in range(iters):
            K.attention_bwd(self.qkr, self.qkv, o, self.do, lse, self.dqkr, self.dqkv, self.B, self.L, self.H, self.D, **kw)
        self.ev[2].record()
        torch.cuda.synchronize()
        return self.ev[0].elapsed_time(self.ev[1]) / iters, self.ev[1].elapsed_time(self.ev[2]) / iters


def set_generated(on):
    v = -1 if on else 0          # -1: the library's unset state (on)
    K.set_attention_fwd64(v)
    K.set_attention_dq64(v)
    K.set_attention_dkv64(v)


def kernel_level(args, dev):
    B, L = 8, L_SEQ
    res = dict(shape_d256=[B, 16, L, 256], shape_d128=[B, 32, L, 128], reps=args.reps, iters=args.iters)
    flops_fwd = 4.0 * B * 16 * L * L * 256       # QK^T and PV; the backward is 2.5 x that (5 matrix products)
    for causal in (False, True):
        c256, c128 = AttnCase(B, 16, L, 256, causal, dev), AttnCase(B, 32, L, 128, causal, dev)
        t = {k: [] for k in ("d256", "d128_8wave", "d128_generated")}
        try:
            for r in range(args.reps + 2):      # two warm-up rounds; the three forms alternate inside a round: drift of the box hits all of them
                set_generated(False)
                a, b = c256.round(args.iters), c128.round(args.iters)
                set_generated(True)
                c = c128.round(args.iters)
                if r >= 2:
                    t["d256"].append(a); t["d128_8wave"].append(b); t["d128_generated"].append(c)
        finally:
            set_generated(True)
        tag = "causal" if causal else "bidirectional"
        med = {k: (statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)) for k, v in t.items()}
        spread = max((max(x[i] for x in v) - min(x[i] for x in v)) / med[k][i] for k, v in t.items() for i in (0, 1))
        frac = 0.5 if causal else 1.0
        res[tag] = dict(
            fwd_ms={k: round(v[0], 4) for k, v in med.items()}, bwd_ms={k: round(v[1], 4) for k, v in med.items()},
            fwd_ratio_d256_over_d128_8wave=round(med["d256"][0] / med["d128_8wave"][0], 3),
            bwd_ratio_d256_over_d128_8wave=round(med["d256"][1] / med["d128_8wave"][1], 3),
            fwd_tflops_d256=round(frac * flops_fwd / (med["d256"][0] * 1e-3) / 1e12, 1),
            bwd_tflops_d256=round(frac * 2.5 * flops_fwd / (med["d256"][1] * 1e-3) / 1e12, 1),
            max_rel_spread=round(spread, 3))
    return res


def xxl_step(args, dev):
    from unidisc_amd import MODEL_PRESETS, Diffusion, make_config

    preset = dict(MODEL_PRESETS["xxl"])
    if args.blocks:
        preset["n_blocks"] = args.blocks
    w = bench.WORKLOADS["unidisc-1.4b-l1280"]      # the 1.4 B workload's data shape and flags (bench.build) on the xxl backbone
    cfg = make_config(**preset, txt_length=TXT, img_length=IMG, norm_type="rms", qk_norm=True, sandwich_normalization=True, modality_embed=True, rope_2d=True,
                      linear_factor=2.0, time_conditioning=False, multimodal_batches=True, force_argmax_valid_indices=True, dropout=0.1, zero_linear_init=False,
                      image_vocab_size=w["image_vocab"], mask_entire_modality=0.1, softmin_snr=5, text_loss_weight=1.0, img_loss_weight=0.5,
                      force_full_attention_mask=True)
    cfg.model.force_text_vocab_size = w["text_vocab"] - 1
    torch.manual_seed(42)
    diff = Diffusion(cfg, None, dev)
    diff.backbone.train()
    B = args.batch
    batch = {k: v.to(dev) for k, v in bench.synthetic_batch("unidisc-1.4b-l1280", B, 42).items()}
    n_params = sum(p.numel() for p in diff.backbone.parameters())
    def drop_grads():   # what an optimizer step + zero_grad(set_to_none=True) leaves: without it every backward holds the previous step's fp32 gradients beside its own
        for p in diff.backbone.parameters():
            p.grad = None

    for i in range(args.warmup):
        diff.training_step(batch, i).loss.backward()
        drop_grads()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = diff.training_step(batch, args.warmup + i)
        out.loss.backward()
        drop_grads()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    tok_s = B * L_SEQ / dt
    f_tok = bench.flops_per_token(preset["n_blocks"], preset["hidden_size"], diff.vocab_size, L_SEQ)
    return dict(mode="xxl_step", preset=preset, B=B, L=L_SEQ, dropout=0.1, steps=args.steps, warmup=args.warmup, params=n_params, ms_per_step=round(dt * 1e3, 2),
                tokens_per_s=round(tok_s, 1), loss=float(out.loss.detach()), flops_per_token=f_tok,
                step_mfu=round(tok_s * f_tok / (bench.PEAK_BF16_DENSE_TFLOPS * 1e12), 4), optimizer="none (fwd + bwd only)",
                max_memory_allocated_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=0, help="override the preset's depth (0 = full depth, 30)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    print(json.dumps(xxl_step(args, dev) if args.step else kernel_level(args, dev)), flush=True)


if __name__ == "__main__":
    main()
