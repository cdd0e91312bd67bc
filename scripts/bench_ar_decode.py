"""KV-cached AR decoding on one MI355X: tokens/s of a full `sample()` (parameterization=ar), device and host-enqueue time per decode step, each skinny-GEMM
shape's time and achieved HBM bandwidth (weights rotated past the last-level cache), and decode attention at p = 256 / 1024 / 4095.  Prints one JSON line.

    python scripts/bench_ar_decode.py [--models s,1.4b] [--batches 8,16,32] [--steps 50]

Models (random weights, AR overrides): UniDisc-S (d 768, 12 heads, 12 blocks, V 40 193, L 384) and 1.4 B (d 2048, 16 heads, 24 blocks, V 48 385, L 1280)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ar_utils import ar_config  # noqa: E402
from oracle.cases import CASES  # noqa: E402
from unidisc_amd import Diffusion  # noqa: E402
from unidisc_amd import kernels as K  # noqa: E402

MODELS = {
    "s": dict(hidden_size=768, n_heads=12, n_blocks=12, txt_length=128, img_length=256, text_vocab_size=32001, vocab_size=40193),
    "1.4b": dict(hidden_size=2048, n_heads=16, n_blocks=24, txt_length=256, img_length=1024, text_vocab_size=32001, vocab_size=48385),
}


def _model(name):
    case = dict(CASES["b_small"], cond_dim=128, batch_size=8, text_loss_weight=None, force_full_attention_mask_loss_only=None, **MODELS[name])
    torch.manual_seed(0)
    diff = Diffusion(ar_config(case), None, "cuda")
    with torch.no_grad():
        for n, p in diff.backbone.named_parameters():
            if p.dim() == 2:
                p.normal_(0, p.shape[-1] ** -0.5)
    diff.backbone.eval()
    return diff


def _events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench_model(name, batches, steps):
    diff = _model(name)
    bb = diff.backbone
    L, d, V = diff.config.model.length, bb.hidden_size, diff.vocab_size
    out = {"L": L, "d": d, "V": V, "blocks": bb.n_blocks, "batches": {}}
    mod = torch.zeros(1, L, dtype=torch.int64, device="cuda")
    mod[:, diff.static_img_sl] = 1
    for B in batches:
        r = {}
        m = mod.expand(B, L).contiguous()
        diff._ar_sampler(B, modality=m, seed=1, bos_token_id=1)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        diff._ar_sampler(B, modality=m, seed=2, bos_token_id=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r["sample_s"] = dt
        r["tokens_per_s"] = B * (L - 1) / dt
        # decode steps at mid-sequence: device time by events, host enqueue time by the wall clock of the enqueue alone
        bb.reset_kv_cache(batch_size=B, seq_len=L - 1, dtype=torch.bfloat16, device="cuda", modality=m)
        p = L // 2
        r["step_device_ms"] = _events_ms(lambda: bb._decode_step(p), steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            bb._decode_step(p)
        r["step_host_enqueue_ms"] = (time.perf_counter() - t0) * 1e3 / steps
        torch.cuda.synchronize()
        bb.reset_kv_cache(set_to_none=True)
        # the skinny GEMM shapes of one step (rows padded to 8).  Each call reads another copy of the weight, round robin over >= 1 GB of copies, so that
        # the weight comes from HBM as in a decode step (a single weight of 8-200 MB would stay in the 256 MB last-level cache between calls)
        Bp = (B + 7) // 8 * 8
        gem = {}
        for tag, N, Kd in (("qkv", 3 * d, d), ("out", d, d), ("up", 4 * d, d), ("down", d, 4 * d), ("head", V, d)):
            a = torch.randn(Bp, Kd, device="cuda").bfloat16()
            Np = (N + 127) // 128 * 128
            ncopy = max(2, -(-(1 << 30) // (Np * Kd * 2)))
            ws = [torch.randn(Np, Kd, device="cuda").bfloat16() for _ in range(ncopy)]
            o = torch.empty(Bp, Np, dtype=torch.bfloat16, device="cuda")
            it = [0]

            def call():
                K.gemm_skinny(a, ws[it[0] % ncopy], out=o, N=N)
                it[0] += 1

            ms = _events_ms(call, 2 * ncopy if ncopy > 25 else 50)
            gem[tag] = {"us": ms * 1e3, "TBps": N * Kd * 2 / (ms * 1e-3) / 1e12, "weight_copies": ncopy}
            del ws
        r["gemm"] = gem
        out["batches"][B] = r
    # decode attention alone (B = 8 rows, the model's heads)
    H, D = bb.n_heads, bb.head_dim
    att = {}
    for p in (256, 1024, 4095):
        Bq, Lmax = 8, 4096
        q = torch.randn(Bq, 2 * d, device="cuda").bfloat16()
        v = torch.randn(Bq, d, device="cuda").bfloat16()
        Kc = torch.zeros(Bq, Lmax, d, dtype=torch.bfloat16, device="cuda")
        Vc = torch.zeros_like(Kc)
        ws = K.attention_decode_ws(Bq, H, D, "cuda")
        o = torch.empty(Bq, d, dtype=torch.bfloat16, device="cuda")
        ms = _events_ms(lambda: K.attention_decode(q[:, :d], q[:, d:], v, Kc, Vc, p, H, D, out=o, ws=ws), 50)
        att[p] = {"us": ms * 1e3, "TBps": 2 * Bq * (p + 1) * d * 2 / (ms * 1e-3) / 1e12}
    out["attention_B8"] = att
    del diff, bb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="s,1.4b")
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    res = {"bench": "ar_decode", "device": torch.cuda.get_device_name(0)}
    for name in args.models.split(","):
        res[name] = bench_model(name, [int(b) for b in args.batches.split(",")], args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
