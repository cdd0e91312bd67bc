"""Top-p sampling on one MI355X: the tensor path against the fused kernels of eval.fused_nucleus, both in this process, the arms alternating round by round.

  rows    per maskgit_nucleus step: `Diffusion._nucleus_draw` + `categorical_sample_rows(given=)` (what the step runs today) against one
          `nucleus_sample_rows` launch, at M = 10 240 and 1 280 [MASK] rows, V = 48 385 (Vt = 32 001), plain and guided; device events around each arm
  ar      the AR sampler at 1.4 B, B = 8 (random weights): wall time of a whole `_ar_sampler` run per decode step (the loop is host-enqueue bound, so the
          wall clock is the number that matters) with argmax, with eval.top_p on the tensor path and with eval.top_p + eval.fused_nucleus

Every figure is the median over the measured rounds after warm-up, with the minimum and maximum beside it (the spread).  Prints one JSON line.

    python scripts/bench_nucleus.py [--parts rows,ar] [--rounds 9] [--ar-rounds 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V, VT, MASK = 48385, 32001, 48384
TOP_P, TEMPERATURE = 0.95, 0.9


def _stats(ms):
    s = sorted(ms)
    return dict(median_ms=round(statistics.median(s), 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), rounds=len(s))


def _alternate(arms, rounds, warmup=2):
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


def bench_rows(rounds):
    from unidisc_amd import Diffusion
    from unidisc_amd import kernels as K

    me = types.SimpleNamespace(vocab_size=V, text_vocab_size=VT, mask_index=MASK)
    ld = (V + 7) // 8 * 8
    out = {}
    for M in (10240, 1280):
        gen = torch.Generator(device="cuda").manual_seed(M)
        logits = (torch.randn(M, ld, device="cuda", generator=gen) * 3.0).bfloat16()
        logits_u = (logits.float() + torch.randn(M, ld, device="cuda", generator=gen)).bfloat16()
        w = torch.full((M,), 1.5, device="cuda")
        modality = (torch.arange(M, device="cuda") % 5 != 0).long()      # 4 of 5 [MASK] rows are image rows, as at 256 + 1024
        for guided in (False, True):
            lu, wr = (logits_u, w) if guided else (None, None)

            def tensor_path():
                given = Diffusion._nucleus_draw(me, logits, lu, wr, modality, TOP_P, TEMPERATURE, 3)
                return K.categorical_sample_rows(logits, V, VT, MASK, modality=modality, restrict=True, given=given, seed=3, logits_u=lu, w=wr)

            def fused():
                return K.nucleus_sample_rows(logits, V, VT, MASK, inv_temperature=1.0, budget=TOP_P * TEMPERATURE, modality=modality, restrict=True, seed=5,
                                             logits_u=lu, w=wr)

            _, _, keep = K.nucleus_sample_rows(logits, V, VT, MASK, inv_temperature=1.0, budget=TOP_P * TEMPERATURE, modality=modality, restrict=True, seed=5,
                                               logits_u=lu, w=wr, want_keep=True)
            r = _alternate({"tensor_path": tensor_path, "fused": fused}, rounds)
            r["kept_median"] = int(keep.median())
            r["fused_over_tensor"] = round(r["fused"]["median_ms"] / r["tensor_path"]["median_ms"], 4)
            out[f"M{M}_{'guided' if guided else 'plain'}"] = r
        del logits, logits_u
        torch.cuda.empty_cache()
    return out


def bench_ar(rounds, B=8):
    from ar_utils import ar_config
    from oracle.cases import CASES
    from unidisc_amd import Diffusion

    case = dict(CASES["b_small"], cond_dim=128, batch_size=8, text_loss_weight=None, force_full_attention_mask_loss_only=None, hidden_size=2048, n_heads=16,
                n_blocks=24, txt_length=256, img_length=1024, text_vocab_size=VT, vocab_size=V)
    torch.manual_seed(0)
    diff = Diffusion(ar_config(case), None, "cuda")
    with torch.no_grad():
        for n, p in diff.backbone.named_parameters():
            if p.dim() == 2:
                p.normal_(0, p.shape[-1] ** -0.5)
    diff.backbone.eval()
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    mod[:, diff.static_img_sl] = 1
    arms = {"argmax": dict(top_p=None, fused_nucleus=False), "top_p_tensor": dict(top_p=TOP_P, fused_nucleus=False),
            "top_p_fused": dict(top_p=TOP_P, fused_nucleus=True)}
    ms = {n: [] for n in arms}
    for r in range(rounds + 1):
        for n, kw in arms.items():
            diff.config.eval.top_p, diff.config.eval.temperature, diff.config.eval.fused_nucleus = kw["top_p"], TEMPERATURE, kw["fused_nucleus"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            diff._ar_sampler(B, modality=mod, seed=r, bos_token_id=1)
            torch.cuda.synchronize()
            if r >= 1:
                ms[n].append((time.perf_counter() - t0) * 1e3 / (L - 1))
    out = {n: _stats(v) for n, v in ms.items()}
    out["steps_per_run"], out["B"] = L - 1, B
    out["fused_over_tensor"] = round(out["top_p_fused"]["median_ms"] / out["top_p_tensor"]["median_ms"], 4)
    out["fused_over_argmax"] = round(out["top_p_fused"]["median_ms"] / out["argmax"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="rows,ar")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--ar-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "V": V, "top_p": TOP_P, "temperature": TEMPERATURE}
    parts = a.parts.split(",")
    if "rows" in parts:
        res["rows"] = bench_rows(a.rounds)
    if "ar" in parts:
        res["ar_step_1.4b_b8"] = bench_ar(a.ar_rounds)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
