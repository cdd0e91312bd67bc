"""eval.ar_decode_graph on one MI355X: a whole AR `sample()` (parameterization=ar, Philox Gumbel, unconditional) with the key off against the key on, in one
process, in alternating rounds (off, on, off, on, ...) after one warm-up of each arm.  Per arm: wall ms per token (the call and the device drained, divided
by the L - 1 tokens; median and p10 - p90 over the rounds) and host ms per token (until the call returns: the enqueue, which with the key on includes the
one capture of the call).  The key-off arm is the sampler as it was before the key existed; a difference counts only beyond that arm's own p10 - p90 spread.
Prints one JSON line (and writes it to --out).

    python scripts/bench_ar_decode_graph.py [--cases s:8,s:32,1.4b:8] [--rounds 7] [--out profiles/ar_decode_graph_bench.json]

Models: those of scripts/bench_ar_decode.py (random weights)."""
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


def _pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, round(q * (len(v) - 1))))]


def _summary(v):
    return dict(median=_pct(v, 0.5), p10=_pct(v, 0.1), p90=_pct(v, 0.9), n=len(v))


def bench_case(diff, B, rounds):
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    mod[:, diff.static_img_sl] = 1
    tokens = L - 1
    wall, host = {False: [], True: []}, {False: [], True: []}
    ledger = {}

    def run(key, seed):
        diff.config.eval.ar_decode_graph = key
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, _ = diff._ar_sampler(B, modality=mod, seed=seed, bos_token_id=1)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ledger[key] = dict(diff.ar_decode_stats)
        return x, (t2 - t0) * 1e3 / tokens, (t1 - t0) * 1e3 / tokens

    x_off, x_on = run(False, 1)[0], run(True, 1)[0]      # warm-up of both arms, and the two arms agree
    same = bool(torch.equal(x_off, x_on))
    for r in range(rounds):
        for key in (False, True):
            _, w, h = run(key, 2 + r)
            wall[key].append(w)
            host[key].append(h)
    diff.config.eval.ar_decode_graph = False
    off, on = _summary(wall[False]), _summary(wall[True])
    return dict(B=B, L=L, tokens=tokens, rounds=rounds, same_tokens=same, ledger_off=ledger[False], ledger_on=ledger[True],
                wall_ms_per_token=dict(off=off, on=on), host_ms_per_token=dict(off=_summary(host[False]), on=_summary(host[True])),
                ratio_on_over_off=on["median"] / off["median"], beyond_off_spread=bool(on["median"] < off["p10"] or on["median"] > off["p90"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="s:8,s:32,1.4b:8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"bench": "ar_decode_graph", "device": torch.cuda.get_device_name(0), "cases": {}}
    cases = [c.split(":") for c in args.cases.split(",")]
    for name in dict.fromkeys(n for n, _ in cases):
        diff = _model(name)
        for n, b in cases:
            if n == name:
                res["cases"][f"{n}:B={b}"] = bench_case(diff, int(b), args.rounds)
        del diff
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
