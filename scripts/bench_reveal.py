"""The sampler step tail on one MI355X: today's tensor statements against `udm_reveal_rows` (eval.fused_reveal), both in this process, device events, warm-up,
the arms alternating round by round (scripts/bench_attention_caching.py::_alternate); median and the 10 % / 90 % quantiles per arm.

    tail     the second half of a maskgit step alone - `Diffusion._maskgit_reveal` (rand-free: explicit Gumbel noise; its `int(num_unmask.max())` host read
             included) plus the x0 write-back, against one `K.reveal_rows` launch with the write-back folded in - at L = 1280, B = 1 / 8 / 64 and L = 4608,
             B = 1 / 2, half the positions [MASK]; the first_hitting tail (`_first_hitting_reveal`) at the same shapes
    sample   a whole Diffusion.sample() of the 1.4 B model (`maskgit`, 16 steps + noise removal, text given) at B = 1 and 8, eval.fused_reveal on against off
             (off is the path as it was)

    python scripts/bench_reveal.py [--parts tail,sample] [--out FILE]        # one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_attention_caching import _alternate  # noqa: E402

WORKLOAD = "unidisc-1.4b-l1280"
SAMPLE_STEPS = 16
TAIL_SHAPES = ((1280, 1), (1280, 8), (1280, 64), (4608, 1), (4608, 2))
MASK, R_TEMP = 48384, 10.0


def _spread(t):
    return round(max((v["p90_ms"] - v["p10_ms"]) / v["median_ms"] for v in t.values()), 4)


def tail():
    import torch

    from unidisc_amd import Diffusion
    from unidisc_amd import kernels as K

    dev = torch.device("cuda", 0)
    rows_out = []
    for L, B in TAIL_SHAPES:
        gen = torch.Generator().manual_seed(L + B)
        x = torch.randint(0, MASK, (B, L), generator=gen)
        x[torch.rand(B, L, generator=gen) < 0.5] = MASK
        x = x.to(dev)
        copy_flag = x != MASK
        rows = (x.reshape(-1) == MASK).nonzero().reshape(-1)
        n = rows.numel()
        tok = torch.randint(0, MASK, (n,), generator=gen).to(dev)
        logp = (-5 * torch.rand(n, generator=gen)).to(dev)
        gumbel = (-torch.log(-torch.log(torch.rand(B, L, generator=gen).clamp(1e-9, 1 - 1e-9)))).to(dev)
        pos_u = torch.rand(B, L, generator=gen).to(dev)
        k = torch.minimum(torch.full((B,), L // 16, dtype=torch.int64, device=dev), (~copy_flag).sum(-1))
        t_col = torch.full((B, 1), 0.5, device=dev)
        t_b = t_col.reshape(-1).contiguous()
        x0 = x.clone()
        for mode in ("maskgit", "first_hitting"):
            if mode == "maskgit":
                tensor = lambda: torch.where(copy_flag, x0, Diffusion._maskgit_reveal(None, x, copy_flag, k, rows, tok, logp, gumbel, 0, R_TEMP, t_col)[0])
                fused = lambda: K.reveal_rows(x, MASK, rows=rows, tok=tok, logp=logp, sched=k, t=t_b, noise=gumbel, r_temp=R_TEMP, x0=x0, x0_unmask=copy_flag)
            else:
                tensor = lambda: torch.where(copy_flag, x0, Diffusion._first_hitting_reveal(x, copy_flag, k, rows, tok, pos_u, 0))
                fused = lambda: K.reveal_rows(x, MASK, rows=rows, tok=tok, sched=k, noise=pos_u, lottery=True, x0=x0, x0_unmask=copy_flag)
            assert torch.equal(tensor(), fused())
            t = _alternate(dict(tensor=tensor, fused=fused), rounds=40, warmup=6)
            rows_out.append(dict(mode=mode, L=L, B=B, mask_rows=n, k=int(k[0]), times=t, fused_over_tensor=round(t["fused"]["median_ms"] / t["tensor"]["median_ms"], 4),
                                 run_to_run_spread=_spread(t)))
    return dict(part="tail", rows=rows_out)


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
        unmask = torch.zeros(B, L, dtype=torch.bool, device=dev)
        unmask[:, :Lt] = True

        def run(key):
            diff.config.eval = Cfg(fused_reveal=key)
            return diff.sample(num_steps=SAMPLE_STEPS, x0=x0, x0_unmask=unmask, modality=mod, seed=3, predictor="maskgit")

        t = _alternate(dict(key_off=lambda: run(False), key_on=lambda: run(True)), rounds=5, warmup=1)
        rows.append(dict(B=B, steps=SAMPLE_STEPS, predictor="maskgit", generated_rows=L - Lt, times=t,
                         key_on_over_key_off=round(t["key_on"]["median_ms"] / t["key_off"]["median_ms"], 4), run_to_run_spread=_spread(t)))
    return dict(part="sample", workload=WORKLOAD, rows=rows)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="tail,sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0))
    for part in a.parts.split(","):
        res[part] = {"tail": tail, "sample": sample}[part]()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
