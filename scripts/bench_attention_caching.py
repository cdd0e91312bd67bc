"""Step times of `eval.attention_caching` with and without eval.attention_caching_read_cache, and udm_attention_fwd_kv alone.

Per shape (1.4 B at B = 8 and B = 1 with L = 256 + 1024; UniDisc-S at B = 64 with L = 128 + 256), in one process, device events, warm-up, the arms alternating
round by round:
    full        one joint step's forward (forward_masked_logits on [B, L])
    build       the build step: the same under ModalityMask(img_drop = 1), with the K / V sink
    text_only   the key-false text step: the backbone on the text slice, text keys alone
    read_cache  the read-cache text step: the text slice against [fresh text keys ; cached image keys]
    kernel      udm_attention_fwd_kv at (Lq = Lt, Lk = L) against udm_attention_fwd at L with the generated forward off (the 8-wave kernel: the same tile body,
                so the ratio of the two times per flop isolates grid fill), both on the engine's layouts
Reports the median and the 10 % / 90 % quantiles per arm, read_cache / full, read_cache / text_only, and the kernel's time per flop over the square kernel's.

    python scripts/bench_attention_caching.py                 # every shape, each in a child process under a time limit; one JSON line
    python scripts/bench_attention_caching.py --one 1.4b      # one model (its batch sizes) in this process

A shape that fails or runs out of time ends the run: nothing more is started on the device after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {"1.4b": ("unidisc-1.4b-l1280", (8, 1)), "small": ("unidisc-s-l384", (64,))}
STEP_LIMIT_S = 420
ROUNDS, WARMUP = 12, 3


def _stats(ms):
    import statistics

    s = sorted(ms)
    return dict(median_ms=round(statistics.median(s), 4), p10_ms=round(s[max(0, len(s) // 10)], 4), p90_ms=round(s[min(len(s) - 1, len(s) * 9 // 10)], 4))


def _alternate(arms, rounds=ROUNDS, warmup=WARMUP):
    """arms: {name: fn}.  Every round runs each arm once, bracketed by its own pair of events; the first `warmup` rounds are dropped."""
    import torch

    ev = {n: [] for n in arms}
    for r in range(rounds + warmup):
        for n, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if r >= warmup:
                ev[n].append((a, b))
    torch.cuda.synchronize()
    return {n: _stats([a.elapsed_time(b) for a, b in pairs]) for n, pairs in ev.items()}


def one(model):
    import torch

    import bench
    from unidisc_amd import kernels as K
    from unidisc_amd.dit import ModalityMask

    workload, batches = MODELS[model]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg, diff = bench.build(workload, dev, 0.0)
    bb = diff.backbone
    bb.eval()
    w = bench.WORKLOADS[workload]
    Lt, L = w["txt_length"], w["txt_length"] + w["img_length"]
    H, D = bb.n_heads, bb.head_dim
    d = H * D
    rows = []
    for B in batches:
        gen = torch.Generator().manual_seed(B)
        mod = torch.zeros(B, L, dtype=torch.int64, device=dev)
        mod[:, Lt:] = 1
        x = torch.where(mod.cpu() == 0, torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen),
                        torch.randint(diff.text_vocab_size, diff.vocab_size, (B, L), generator=gen)).to(dev)
        x = torch.where(torch.rand(B, L, generator=gen).to(dev) < 0.5, torch.full_like(x, diff.mask_index), x)      # half the positions still [MASK]
        x_text, mod_text = x[:, :Lt].contiguous(), mod[:, :Lt].contiguous()
        bm = ModalityMask(torch.zeros(B, dtype=torch.bool, device=dev), torch.ones(B, dtype=torch.bool, device=dev), Lt)
        with torch.no_grad():
            bb.set_flex_attention_cache(B, L, dev, None, read_cache=True)
            bb.forward_masked_logits(x, None, modality=mod, block_mask=bm, modality_cache="build")
            steps = _alternate(dict(
                full=lambda: bb.forward_masked_logits(x, None, modality=mod),
                build=lambda: bb.forward_masked_logits(x, None, modality=mod, block_mask=bm, modality_cache="build"),
                text_only=lambda: bb.forward_masked_logits(x_text, None, modality=mod_text),
                read_cache=lambda: bb.forward_masked_logits(x_text, None, modality=mod_text, modality_cache="read")))
            bb.reset_kv_cache()
        # the kernel alone, on the engine's layouts: q | k in [M, 2 d], v in [M, 3 d]; the cache [B, L, d]
        qkr = torch.randn(B * L, 2 * d, device=dev).to(torch.bfloat16)
        qkr[:, :d] *= K.attention_q_scale(D)
        qkv = torch.randn(B * L, 3 * d, device=dev).to(torch.bfloat16)
        kc, vc = qkr.view(B, L, 2 * d)[:, :, d:].contiguous(), qkv.view(B, L, 3 * d)[:, :, 2 * d:].contiguous()
        q_text = qkr.view(B, L, 2 * d)[:, :Lt].reshape(B * Lt, 2 * d)[:, :d]
        K.set_attention_fwd64(0)
        try:
            kern = _alternate(dict(fwd_kv=lambda: K.attention_fwd_kv(q_text, kc, vc, B, Lt, L, H, D, q_prescaled=True),
                                   fwd_square_8wave=lambda: K.attention_fwd(qkr, qkv, B, L, H, D, q_prescaled=True)), rounds=3 * ROUNDS, warmup=2 * WARMUP)
        finally:
            K.set_attention_fwd64(-1)
        fl_kv, fl_sq = 4.0 * B * H * Lt * L * D, 4.0 * B * H * L * L * D
        for n, fl in (("fwd_kv", fl_kv), ("fwd_square_8wave", fl_sq)):
            kern[n]["tflops"] = round(fl / (kern[n]["median_ms"] * 1e-3) / 1e12, 2)
            kern[n]["workgroups"] = (((Lt if n == "fwd_kv" else L) + 127) // 128) * B * H
        per_flop = (kern["fwd_kv"]["median_ms"] / fl_kv) / (kern["fwd_square_8wave"]["median_ms"] / fl_sq)
        spread = max((k["p90_ms"] - k["p10_ms"]) / k["median_ms"] for k in kern.values())
        rows.append(dict(workload=workload, B=B, L=L, Lt=Lt, H=H, D=D, steps=steps, kernel=kern,
                         read_cache_over_full=round(steps["read_cache"]["median_ms"] / steps["full"]["median_ms"], 4),
                         read_cache_over_text_only=round(steps["read_cache"]["median_ms"] / steps["text_only"]["median_ms"], 4),
                         kernel_time_per_flop_over_square=round(per_flop, 3), kernel_run_to_run_spread=round(spread, 3)))
        del qkr, qkv, kc, vc
    print(json.dumps(dict(model=model, device=torch.cuda.get_device_name(0), rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default=None, choices=sorted(MODELS))
    a = ap.parse_args()
    if a.one:
        return one(a.one)
    out_rows, failed = [], False
    for model in MODELS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", model], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            out_rows.append(dict(model=model, error=f"time limit of {STEP_LIMIT_S} s"))
            failed = True
            break
        if out.returncode != 0:
            out_rows.append(dict(model=model, error=f"exit status {out.returncode}", stderr=out.stderr[-800:]))
            failed = True
            break
        out_rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(bench="attention_caching", results=out_rows)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
