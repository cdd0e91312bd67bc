"""Times of conditional sampling with and without eval.conditioning_cache, and of udm_attention_fwd_kv_split against udm_attention_fwd_kv.

In one process per part, device events, warm-up, the arms alternating round by round (scripts/bench_attention_caching.py::_alternate):
    sample   a whole Diffusion.sample() of the 1.4 B model (L = 256 + 1024) with the `maskgit` predictor, the key on and off in the same run: B = 1 and 8,
             both directions (text given -> the 1024 image positions are generated; image given -> the 256 text positions), with and without eval.cfg
    kernel   udm_attention_fwd_kv_split (the plan's split count, splits = 0) against udm_attention_fwd_kv at H = 16, D = 128, 256 x 1280 and 1024 x 1280,
             B = 1 / 2 / 8, on the engine's layouts (q = columns of [M, 2 d], the cache [B, L, d])
Reports the median and the 10 % / 90 % quantiles per arm, key_on / key_off, split / unsplit with the split count the plan chose and the run-to-run spread
((p90 - p10) / median, the larger of the two arms): a shape the plan splits and where split / unsplit exceeds 1 + spread is a shape the plan should leave alone.

    python scripts/bench_conditioning_cache.py                  # both parts, each in a child process under a time limit; one JSON line
    python scripts/bench_conditioning_cache.py --one kernel     # one part in this process

A part that fails or runs out of time ends the run: nothing more is started on the device after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_attention_caching import _alternate  # noqa: E402

PARTS = ("kernel", "sample")
STEP_LIMIT_S = 420
WORKLOAD = "unidisc-1.4b-l1280"
SAMPLE_STEPS = 16
KERNEL_SHAPES = ((256, 1280), (1024, 1280))
KERNEL_BATCHES = (1, 2, 8)


def kernel():
    import torch

    from unidisc_amd import kernels as K

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    H, D = 16, 128
    d = H * D
    rows = []
    for Lq, L in KERNEL_SHAPES:
        for B in KERNEL_BATCHES:
            qkr = torch.randn(B * Lq, 2 * d, device=dev).to(torch.bfloat16)
            qkr[:, :d] *= K.attention_q_scale(D)
            kc = torch.randn(B, L, d, device=dev).to(torch.bfloat16)
            vc = torch.randn(B, L, d, device=dev).to(torch.bfloat16)
            q = qkr[:, :d]
            S, n_ws = K.attention_kv_split_plan(B, Lq, L, H, D)
            ws = K.attention_kv_split_ws(B, Lq, L, H, D, dev)
            arms = dict(unsplit=lambda: K.attention_fwd_kv(q, kc, vc, B, Lq, L, H, D, q_prescaled=True),
                        split=lambda: K.attention_fwd_kv_split(q, kc, vc, B, Lq, L, H, D, q_prescaled=True, ws=ws))
            forced = {}
            for s_forced in (2, 4, 8):      # (for the plan's rule: what other counts would cost at this shape)
                if s_forced != S:
                    ws_f = K.attention_kv_split_ws(B, Lq, L, H, D, dev, splits=s_forced)
                    forced[s_forced] = ws_f
                    arms[f"split_{s_forced}"] = (lambda s_=s_forced, w_=ws_f: K.attention_fwd_kv_split(q, kc, vc, B, Lq, L, H, D, q_prescaled=True, ws=w_, splits=s_))
            t = _alternate(arms, rounds=36, warmup=6)
            fl = 4.0 * B * H * Lq * L * D
            for v in t.values():
                v["tflops"] = round(fl / (v["median_ms"] * 1e-3) / 1e12, 2)
            spread = max((t[n]["p90_ms"] - t[n]["p10_ms"]) / t[n]["median_ms"] for n in ("unsplit", "split"))
            rows.append(dict(B=B, H=H, D=D, Lq=Lq, Lk=L, plan_splits=S, ws_floats=n_ws, unsplit_workgroups=((Lq + 127) // 128) * B * H, times=t,
                             split_over_unsplit=round(t["split"]["median_ms"] / t["unsplit"]["median_ms"], 4), run_to_run_spread=round(spread, 4)))
            del qkr, kc, vc, ws, forced
    print(json.dumps(dict(part="kernel", device=torch.cuda.get_device_name(0), rows=rows)))


def sample():
    import torch

    import bench
    from unidisc_amd.config import Cfg

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg, diff = bench.build(WORKLOAD, dev, 0.0)
    diff.backbone.eval()
    w = bench.WORKLOADS[WORKLOAD]
    Lt, L = w["txt_length"], w["txt_length"] + w["img_length"]
    rows = []
    for B in (1, 8):
        gen = torch.Generator().manual_seed(B)
        mod = torch.zeros(B, L, dtype=torch.int64)
        mod[:, Lt:] = 1
        x0 = torch.where(mod == 0, torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen), torch.randint(diff.text_vocab_size, diff.vocab_size, (B, L), generator=gen))
        x0, mod = x0.to(dev), mod.to(dev)
        for given in ("image", "text"):
            unmask = torch.zeros(B, L, dtype=torch.bool, device=dev)
            unmask[:, (slice(0, Lt) if given == "text" else slice(Lt, L))] = True
            for guidance in (None, 2.0):
                def run(key):
                    diff.config.eval = Cfg(cfg=guidance, conditioning_cache=key)
                    return diff.sample(num_steps=SAMPLE_STEPS, x0=x0, x0_unmask=unmask, modality=mod, seed=3, predictor="maskgit")

                t = _alternate(dict(key_off=lambda: run(False), key_on=lambda: run(True)), rounds=4, warmup=1)
                spread = max((v["p90_ms"] - v["p10_ms"]) / v["median_ms"] for v in t.values())
                rows.append(dict(B=B, given=given, generated_rows=L - Lt if given == "text" else Lt, cfg=guidance, steps=SAMPLE_STEPS, predictor="maskgit", times=t,
                                 key_on_over_key_off=round(t["key_on"]["median_ms"] / t["key_off"]["median_ms"], 4), run_to_run_spread=round(spread, 4)))
    print(json.dumps(dict(part="sample", workload=WORKLOAD, device=torch.cuda.get_device_name(0), rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default=None, choices=PARTS)
    a = ap.parse_args()
    if a.one:
        return {"kernel": kernel, "sample": sample}[a.one]()
    out_rows, failed = [], False
    for part in PARTS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", part], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            out_rows.append(dict(part=part, error=f"time limit of {STEP_LIMIT_S} s"))
            failed = True
            break
        if out.returncode != 0:
            out_rows.append(dict(part=part, error=f"exit status {out.returncode}", stderr=out.stderr[-800:]))
            failed = True
            break
        out_rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(bench="conditioning_cache", results=out_rows)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
