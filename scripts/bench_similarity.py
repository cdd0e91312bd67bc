"""Zero-shot likelihood scoring on the 1.4 B workload (B = 8 pairs, L = 1280 = 256 text + 1024 image, V = 48385, T = 32 timesteps): the fused path
(`Diffusion.get_similarity`: head on the contributing rows, udm_subs_logp_rows, udm_likelihood_scores) against the unfused composition in the same process
(`Diffusion.forward` -> [B, L, V] SUBS log-probs, or two [B, L, V] logits + an fp32 mix under guidance, then the reference's tensor statements,
model_eval.py:320-370), guided (eval.cfg = 1.5) and unguided, with eval.similarity_timesteps_per_pass k in {1, 4}.  Reports ms per call and peak memory.

    python scripts/bench_similarity.py            # every configuration, each in a child process of its own under a time limit; one JSON line
    python scripts/bench_similarity.py --one guided=1,k=4   # one configuration in this process

A configuration that fails or runs out of time ends the run: nothing more is started on the device after it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, LT, T = 8, 1280, 256, 32
CONFIGS = [dict(guided=g, k=k) for g in (0, 1) for k in (1, 4)]
STEP_LIMIT_S = 240


def one(guided, k):
    import torch

    import bench
    from unidisc_amd.config import Cfg

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg, diff = bench.build("unidisc-1.4b-l1280", dev, 0.0)
    diff.backbone.eval()
    mask, Vt = diff.mask_index, diff.text_vocab_size
    modality = torch.zeros(B, L, dtype=torch.int64, device=dev)
    modality[:, LT:] = 1
    x0 = torch.randint(0, Vt - 1, (B, L), device=dev)
    x0[:, LT:] = torch.randint(Vt, diff.vocab_size, (B, L - LT), device=dev)
    pad = 0
    x0[:, LT - 32:LT] = pad                                  # a padded caption tail
    batch = dict(modality=modality, input_ids=x0, attention_mask=x0 != pad)
    diff.config.eval = Cfg(cfg=1.5 if guided else None, pad_token_id=pad, similarity_timesteps_per_pass=k)
    diff.config.model.txt_length = LT
    cond_mask = torch.zeros_like(x0, dtype=torch.bool)
    cond_mask[:, :LT] = True
    pad_mask = x0 == pad
    full_mask = torch.full_like(x0, mask)

    def fused():
        return diff.get_similarity(x0, batch, num_timesteps=T, txt_cond=True)

    @torch.no_grad()
    def unfused():
        times = torch.linspace(0, 1, steps=T + 2)[1:-1].to(dev).to(torch.float32)
        acc = []
        for i in range(T):
            t = times[i].expand(B)
            sigma, dsigma = diff.noise(t)
            xt = diff.q_xt(x0, 1 - torch.exp(-sigma[:, None]), batch=batch)
            cond = torch.where(cond_mask, x0, xt)
            if guided:
                lc = diff.forward(cond, None, batch=batch, modality=modality, return_logits=True)
                lu = diff.forward(torch.where(cond_mask, full_mask, xt), None, batch=batch, modality=modality, return_logits=True)
                w = diff._similarity_cfg_weight(t)[:, None, None]
                out = diff._subs_parameterization(((1 + w) * lc.float() - w * lu.float()).to(torch.bfloat16), xt=xt, batch=batch, modality=modality)
            else:
                out = diff.forward(cond, None, batch=batch, modality=modality)
            log_p = torch.gather(out, -1, x0[:, :, None]).squeeze(-1).float()
            log_p = torch.where(pad_mask | cond_mask, torch.zeros_like(log_p), log_p)
            acc.append((-log_p * (dsigma / torch.expm1(sigma))[:, None]).sum(-1) / (~pad_mask).sum(-1))
        return torch.stack(acc).mean(0)

    def timed(fn, n=2):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20, out

    base = torch.cuda.memory_allocated() / 2 ** 20
    res = dict(guided=bool(guided), k=k, model_mib=round(base, 1))
    ms, peak, s_f = timed(fused)
    res.update(fused_ms=round(ms, 1), fused_peak_mib=round(peak, 1))
    if k == 1:   # (the unfused composition has no k)
        ms, peak, s_u = timed(unfused)
        res.update(unfused_ms=round(ms, 1), unfused_peak_mib=round(peak, 1))
    res["score_mean"] = round(float(s_f.mean()), 4)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", default=None)
    a = ap.parse_args()
    if a.one:
        kv = dict(p.split("=") for p in a.one.split(","))
        return one(int(kv["guided"]), int(kv["k"]))
    rows = []
    for c in CONFIGS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"guided={c['guided']},k={c['k']}"], capture_output=True, text=True,
                                 timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            rows.append(dict(c, error=f"time limit of {STEP_LIMIT_S} s"))
            break
        if out.returncode != 0:
            rows.append(dict(c, error=f"exit status {out.returncode}", stderr=out.stderr[-600:]))
            break
        rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(dict(workload="unidisc-1.4b-l1280", B=B, L=L, T=T, rows=rows)))
    return 1 if any("error" in r for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main())
