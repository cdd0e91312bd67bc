"""The chunked KV-cached forward of the AR baseline on one MI355X (DIT._forward_chunk, udm_attention_fwd_kv_causal, eval.ar_chunk_given).  Device times by
events, every shape warmed up, the arms of a comparison alternating inside one process; the result goes to profiles/ar_chunked_bench.json and, as one JSON
line, to stdout.

    python scripts/bench_ar_chunked.py [--models s,1.4b] [--rows 8,64] [--parts a,b,c] [--rounds 7] [--out profiles/ar_chunked_bench.json]

  (a) chunk   one chunk forward of n in {2, 4, 8, 16, 32, 64, 128, 256} tokens at p = 256 against n decode steps (positions p .. p + n - 1), at 8 and 64 cached
              rows.  `min_tokens`: the smallest n from which on the chunk is faster at every larger measured n too - the source of eval.ar_chunk_min_tokens.
  (b) kernel  udm_attention_fwd_kv_causal against udm_attention_fwd_kv at the same (Lq, Lk) = (n, 256 + n), and against the square causal udm_attention_fwd
              at Lq = Lk; `spread` is (p90 - p10) / median of repeated identical calls, the noise a difference must exceed to mean anything.
  (c) sample  Diffusion.sample() on an inpainting pattern - the text prefix and every second 64-token span of the image given - with the key on and off.

Models (random weights, AR overrides) as in scripts/bench_ar_decode.py: UniDisc-S (d 768, 12 heads, 12 blocks, L 384) and 1.4 B (d 2048, 16 heads, 24 blocks,
L 1280).  A shape that does not fit (p + n past the cache of UniDisc-S) is reported as "not measured"."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ar_decode import _model  # noqa: E402
from unidisc_amd import kernels as K  # noqa: E402

P0 = 256
CHUNKS = (2, 4, 8, 16, 32, 64, 128, 256)
WARMUP = 2


def _stats(ms):
    s = sorted(ms)
    med = statistics.median(s)
    p10, p90 = s[max(0, len(s) // 10)], s[min(len(s) - 1, len(s) * 9 // 10)]
    return dict(median_ms=round(med, 4), p10_ms=round(p10, 4), p90_ms=round(p90, 4), spread=round((p90 - p10) / med, 4))


def _alternate(arms, rounds):
    """arms: {name: fn}.  Every round runs each arm once, bracketed by its own pair of events; the first WARMUP rounds are dropped."""
    ev = {n: [] for n in arms}
    for r in range(rounds + WARMUP):
        for n, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if r >= WARMUP:
                ev[n].append((a, b))
    torch.cuda.synchronize()
    return {n: _stats([a.elapsed_time(b) for a, b in pairs]) for n, pairs in ev.items()}


def _modality(diff, B):
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    mod[:, diff.static_img_sl] = 1
    return mod


def part_chunk(diff, rows_list, rounds):
    bb = diff.backbone
    L = diff.config.model.length
    out = {}
    for B in rows_list:
        mod = _modality(diff, B)
        gen = torch.Generator().manual_seed(B)
        x = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to("cuda")
        bb.reset_kv_cache(batch_size=B, seq_len=L - 1, dtype=torch.bfloat16, device="cuda", modality=mod)
        Lmax = bb._kv.Lmax
        bb._prefill(x[:, :min(Lmax, P0 + max(CHUNKS))], None, last_only=True)      # every slot a timed call reads holds a real key
        res = {}
        for n in CHUNKS:
            if P0 + n > Lmax:
                res[n] = "not measured (p + n past the cache)"
                continue
            ids = x[:, P0:P0 + n]

            def steps():
                for k in range(n):
                    bb._decode_step(P0 + k)

            t = _alternate(dict(chunk=lambda: bb._forward_chunk(ids, None, P0, last_only=True), decode_steps=steps), rounds if n <= 64 else max(3, rounds // 2))
            t["chunk_over_decode"] = round(t["chunk"]["median_ms"] / t["decode_steps"]["median_ms"], 4)
            res[n] = t
        measured = [n for n in CHUNKS if isinstance(res[n], dict)]
        faster = [n for n in measured if all(res[k]["chunk_over_decode"] < 1.0 for k in measured if k >= n)]
        out[B] = dict(p=P0, chunks=res, min_tokens=min(faster) if faster else None)
        bb.reset_kv_cache(set_to_none=True)
    return out


def part_kernel(diff, rows_list, rounds):
    bb = diff.backbone
    H, D = bb.n_heads, bb.head_dim
    d = H * D
    out = {}
    for B in rows_list:
        res = {}
        for n in CHUNKS:
            Lq, Lk = n, P0 + n
            qkr = torch.randn(B * Lq, 2 * d, device="cuda").to(torch.bfloat16)
            qkr[:, :d] *= K.attention_q_scale(D)
            kc = torch.randn(B, Lk + 64, d, device="cuda").to(torch.bfloat16)
            vc = torch.randn(B, Lk + 64, d, device="cuda").to(torch.bfloat16)
            o = torch.empty(B * Lq, d, dtype=torch.bfloat16, device="cuda")
            q = qkr[:, :d]
            t = _alternate(dict(causal=lambda: K.attention_fwd_kv_causal(q, kc, vc, B, Lq, Lk, H, D, q_prescaled=True, out=o),
                                bidirectional=lambda: K.attention_fwd_kv(q, kc, vc, B, Lq, Lk, H, D, q_prescaled=True, out=o),
                                causal_again=lambda: K.attention_fwd_kv_causal(q, kc, vc, B, Lq, Lk, H, D, q_prescaled=True, out=o)), 3 * rounds)
            t["causal_over_bidirectional"] = round(t["causal"]["median_ms"] / t["bidirectional"]["median_ms"], 4)
            t["identical_calls_ratio"] = round(t["causal_again"]["median_ms"] / t["causal"]["median_ms"], 4)
            res[f"{Lq}x{Lk}"] = t
        for Ls in (256, 1024):      # the square case against the square causal kernel (q | k in [M, 2 d], v in [M, 3 d]; the generated forward has no causal form)
            qkr = torch.randn(B * Ls, 2 * d, device="cuda").to(torch.bfloat16)
            qkr[:, :d] *= K.attention_q_scale(D)
            qkv = torch.randn(B * Ls, 3 * d, device="cuda").to(torch.bfloat16)
            kc = qkr.view(B, Ls, 2 * d)[:, :, d:].contiguous()
            vc = qkv.view(B, Ls, 3 * d)[:, :, 2 * d:].contiguous()
            q = qkr[:, :d]
            t = _alternate(dict(kv_causal=lambda: K.attention_fwd_kv_causal(q, kc, vc, B, Ls, Ls, H, D, q_prescaled=True),
                                square_causal=lambda: K.attention_fwd(qkr, qkv, B, Ls, H, D, q_prescaled=True, causal=True)), 3 * rounds)
            t["kv_causal_over_square_causal"] = round(t["kv_causal"]["median_ms"] / t["square_causal"]["median_ms"], 4)
            res[f"square_{Ls}"] = t
        out[B] = res
    return out


def part_sample(diff, rows_list, rounds):
    L, Lt = diff.config.model.length, diff.config.model.txt_length
    diff.tokenizer = types.SimpleNamespace(bos_token_id=1)
    out = {}
    for B in rows_list:
        mod = _modality(diff, B)
        gen = torch.Generator().manual_seed(B)
        x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to("cuda")
        unmask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
        unmask[:, :Lt] = True
        for s in range(Lt + 64, L, 128):      # every second 64-token span of the image
            unmask[:, s:s + 64] = True
        given = int(unmask[0].sum())

        def run(on):
            diff.config.eval.ar_chunk_given = on
            return diff.sample(x0=x0, x0_unmask=unmask, modality=mod, seed=3)

        try:
            t = _alternate(dict(key_on=lambda: run(True), key_off=lambda: run(False)), max(3, rounds // 2))
        finally:
            diff.config.eval.ar_chunk_given = False
        t["on_over_off"] = round(t["key_on"]["median_ms"] / t["key_off"]["median_ms"], 4)
        t["given_columns"], t["length"], t["min_tokens"] = given, L, diff.AR_CHUNK_MIN_TOKENS
        out[B] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="s,1.4b")
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ar_chunked_bench.json"))
    args = ap.parse_args()
    rows = [int(b) for b in args.rows.split(",")]
    parts = args.parts.split(",")
    res = {"bench": "ar_chunked", "device": torch.cuda.get_device_name(0), "p": P0, "rounds": args.rounds}
    for name in args.models.split(","):
        diff = _model(name)
        r = {"d": diff.backbone.hidden_size, "heads": diff.backbone.n_heads, "blocks": diff.backbone.n_blocks, "L": diff.config.model.length}
        with torch.no_grad():
            if "a" in parts:
                r["chunk_vs_decode_steps"] = part_chunk(diff, rows, args.rounds)
            if "b" in parts:
                r["kernel"] = part_kernel(diff, rows, args.rounds)
            if "c" in parts:
                r["sample_inpainting"] = part_sample(diff, rows[:1], args.rounds)      # (one row count: a sample() is thousands of launches)
        res[name] = r
        del diff
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
