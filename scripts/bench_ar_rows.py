"""The AR sampler at 128 cache rows on one MI355X (random weights, the models of scripts/bench_ar_decode.py), one process per --model.

Arms, in alternating rounds after one warm-up of each (wall ms of the call(s) with the device drained; median, p10, p90 over the rounds):
  unguided   one sample() of 128 rows                 against two consecutive calls of 64 rows (the only way below 65 cache rows)
  guided     one guided sample() of 64 samples (128 cache rows)   against two guided calls of 32 samples (64 cache rows each)
(eval.ar_decode_graph as --decode-graph says, default on: the token loop is then one graph launch per token and the wall time follows the device.)

For the 128-row and the 64-row cache: device ms of one captured decode step replayed at p = 256, and device us of each of the step's five skinny GEMM
shapes alone (each call on another copy of the weight, round robin over >= 1 GB, so that it comes from HBM) - at 128 rows as one call, the two-row-group
kernel, and as two calls of the 64-row kernel on the row halves, which is what a shape that loses would be dispatched as.  Prints one JSON line; --out
merges it into a JSON file keyed by model.

    python scripts/bench_ar_rows.py --model s|1.4b [--rounds 5] [--decode-graph 1] [--out profiles/ar_decode_rows_bench.json]

On a shared machine: one process at a time, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 420 python scripts/bench_ar_rows.py --model s --out profiles/ar_decode_rows_bench.json && \\
    timeout -k 10 540 python scripts/bench_ar_rows.py --model 1.4b --out profiles/ar_decode_rows_bench.json"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ar_decode import _model  # noqa: E402
from unidisc_amd import kernels as K  # noqa: E402


def _pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, round(q * (len(v) - 1))))]


def _summary(v):
    return dict(median=_pct(v, 0.5), p10=_pct(v, 0.1), p90=_pct(v, 0.9), n=len(v))


def _verdict(one, two):
    """the one-call arm against the two-call arm: faster below its p10, slower above its p90"""
    return "faster" if one["median"] < two["p10"] else ("slower" if one["median"] > two["p90"] else "equal within spread")


def _events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _mod(diff, B):
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    mod[:, diff.static_img_sl] = 1
    return mod


def bench_sample(diff, guided, rounds):
    """wall ms: one call on 128 cache rows against two calls on 64 cache rows each"""
    ev, m = diff.config.eval, diff.config.model
    L, Lt = m.length, m.txt_length
    n_one = 64 if guided else 128
    ev.cfg = 1.5 if guided else None
    ev.force_cfg_value = bool(guided)
    gen = torch.Generator().manual_seed(3)
    x0 = unmask = None
    if guided:      # the text is given, the image is generated under guidance
        x0 = torch.randint(0, diff.text_vocab_size - 1, (n_one, L), generator=gen).cuda()
        unmask = torch.zeros(n_one, L, dtype=torch.bool, device="cuda")
        unmask[:, :Lt] = True
    mod = _mod(diff, n_one)

    def call(lo, hi, seed):
        kw = dict(x0=x0[lo:hi], x0_unmask=unmask[lo:hi]) if guided else {}
        return diff._ar_sampler(hi - lo, modality=mod[lo:hi], seed=seed, bos_token_id=1, **kw)[0]

    def run(parts, seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xs = [call(lo, hi, seed) for lo, hi in parts]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, xs

    one, two = [(0, n_one)], [(0, n_one // 2), (n_one // 2, n_one)]
    run(one, 1), run(two, 1)      # warm-up of both arms
    wall = {"one": [], "two": []}
    for r in range(rounds):
        wall["one"].append(run(one, 2 + r)[0])
        wall["two"].append(run(two, 2 + r)[0])
    ev.cfg, ev.force_cfg_value = None, False
    s1, s2 = _summary(wall["one"]), _summary(wall["two"])
    tokens = n_one * (L - 1 - (Lt - 1 if guided else 0))
    return dict(samples=n_one, cache_rows_one_call=128, cache_rows_two_calls=64, L=L, generated_tokens=tokens, rounds=rounds,
                wall_ms=dict(one_call=s1, two_calls=s2), ratio_one_over_two=s1["median"] / s2["median"], verdict=_verdict(s1, s2),
                tokens_per_s=dict(one_call=tokens / (s1["median"] * 1e-3), two_calls=tokens / (s2["median"] * 1e-3)))


def bench_step(diff, rows, rounds, reps=30, p=256):
    """device ms of the captured decode step replayed at position p (a device-side fill of the position in front of every replay)"""
    bb = diff.backbone
    L = diff.config.model.length
    bb.reset_kv_cache(batch_size=rows, seq_len=L - 1, dtype=torch.bfloat16, device="cuda", modality=_mod(diff, rows))
    bb.set_decode_position(p)
    g = bb.capture_decode_step(None)

    def step():
        bb.set_decode_position(p)
        g.replay()

    step()
    torch.cuda.synchronize()
    ms = [_events_ms(step, reps) for _ in range(rounds)]
    g = None
    bb.reset_kv_cache(set_to_none=True)
    return _summary(ms)


def bench_gemms(diff, rounds):
    """device us per shape: 64 rows (the 64-row kernel), 128 rows in one call (two row groups), 128 rows as two calls of the 64-row kernel on the halves"""
    d, V = diff.backbone.hidden_size, diff.vocab_size
    out = {}
    for tag, N, Kd, epi in (("qkv", 3 * d, d, K.EPI_NONE), ("out", d, d, K.EPI_NONE), ("up", 4 * d, d, K.EPI_BIAS_GELU), ("down", d, 4 * d, K.EPI_BIAS),
                            ("head", V, d, K.EPI_BIAS)):
        a = torch.randn(128, Kd, device="cuda").bfloat16()
        Np = (N + 127) // 128 * 128
        ncopy = max(2, -(-(1 << 30) // (Np * Kd * 2)))
        ws_ = [torch.randn(Np, Kd, device="cuda").bfloat16() for _ in range(ncopy)]
        bias = torch.randn(Np, device="cuda") if epi != K.EPI_NONE else None
        o = torch.empty(128, Np, dtype=torch.bfloat16, device="cuda")
        gws = torch.empty(max(K.skinny_ws_elems(128, N, Kd), 4), dtype=torch.float32, device="cuda")
        it = [0]
        kw = dict(N=N, epilogue=epi, bias=bias, ws=gws)

        def rows64():
            K.gemm_skinny(a[:64], ws_[it[0] % ncopy], out=o[:64], **kw)
            it[0] += 1

        def rows128():
            K.gemm_skinny(a, ws_[it[0] % ncopy], out=o, **kw)
            it[0] += 1

        def halves():
            w = ws_[it[0] % ncopy]
            K.gemm_skinny(a[:64], w, out=o[:64], **kw)
            K.gemm_skinny(a[64:], w, out=o[64:], **kw)
            it[0] += 1

        arms = dict(rows64=rows64, rows128_one_call=rows128, rows128_two_calls=halves)
        reps = max(ncopy, 20)
        us = {k: [] for k in arms}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, fn in arms.items():
                us[k].append(_events_ms(fn, reps) * 1e3)
        r = {k: _summary(v) for k, v in us.items()}
        r.update(N=N, K=Kd, weight_copies=ncopy, weight_TBps_one_call=N * Kd * 2 / (r["rows128_one_call"]["median"] * 1e-6) / 1e12,
                 weight_TBps_rows64=N * Kd * 2 / (r["rows64"]["median"] * 1e-6) / 1e12,
                 one_call_against_two_calls=_verdict(r["rows128_one_call"], r["rows128_two_calls"]),
                 one_call_over_two_calls=r["rows128_one_call"]["median"] / r["rows128_two_calls"]["median"],
                 one_call_over_rows64=r["rows128_one_call"]["median"] / r["rows64"]["median"])
        out[tag] = r
        del ws_
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s", choices=["s", "1.4b"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode-graph", type=int, default=1)
    ap.add_argument("--parts", default="gemm,step,unguided,guided")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    diff = _model(args.model)
    diff.config.eval.ar_decode_graph = bool(args.decode_graph)
    res = {"device": torch.cuda.get_device_name(0), "decode_graph": bool(args.decode_graph), "L": diff.config.model.length,
           "d": diff.backbone.hidden_size, "V": diff.vocab_size, "blocks": diff.backbone.n_blocks}
    for part, key, fn in (("gemm", "gemm_us", lambda: bench_gemms(diff, args.rounds)),
                          ("step", "step_ms_p256", lambda: {str(rows): bench_step(diff, rows, args.rounds) for rows in (64, 128)}),
                          ("unguided", "unguided", lambda: bench_sample(diff, False, args.rounds)),
                          ("guided", "guided", lambda: bench_sample(diff, True, args.rounds))):
        if part in parts:
            res[key] = fn()
            print(f"{args.model} {part}: {json.dumps(res[key])}", file=sys.stderr, flush=True)
    print(json.dumps({"bench": "ar_decode_rows", args.model: res}))
    if args.out:
        whole = {"bench": "ar_decode_rows"}
        if os.path.exists(args.out):
            with open(args.out) as f:
                whole = json.load(f)
        whole.setdefault(args.model, {}).update(res)
        with open(args.out, "w") as f:
            f.write(json.dumps(whole, indent=1) + "\n")


if __name__ == "__main__":
    main()
