"""Golden vectors of the AR baseline's SAMPLER (`_ar_sampler`, model_eval.py:2736-2822) from the IMPORTED reference, CPU fp32.  Build container only
(the reference does not travel):

    python scripts/make_golden_ar_sampler.py     # writes tests/golden/ar_sampler_{uncond,cond,cfg}.npz

TEST INFRASTRUCTURE.  The model is oracle/cases.py `b_small` (1-D rope, force_argmax_valid_indices) with the AR overrides of scripts/make_golden_ar.py, the
same parameters as tests/golden/ar_b_small.npz, evaluated (eval mode).  The reference's own `_ar_sampler` runs with a tokenizer shim that supplies the BOS
id; its Gumbel draw (`torch.distributions.Gumbel(0, 1).sample`) and, every step, the argument of its `argmax` (next + noise[:, i]) are captured by
wrapping those two calls.  Three runs: unconditional; text-conditioned (x0_unmask = the text positions of the case batch); the same with eval.cfg = 1.5 and
eval.force_cfg_value = true.  Each runs with model.use_kv_cache = false (the reference semantics: a prefix forward per step; recorded) and, as a
cross-check, = true (the reference's cached path: whether it agrees is recorded as meta/kv_cache_agrees).

Recorded per run: noise [B, L-1, V], the final x and nfe, per step the fp32 `next` row ([B, L-1, V], after guidance and the modality restriction) and the
margin between the top two values of next + noise ([B, L-1]), the conditioning (x0, x0_unmask), the modality map and the BOS id.

2-D rope (c_large, not recorded here; tests/golden/ar_c_large.npz holds the reference's full-sequence logits): `find_rope_2d_quirk()` runs the reference
backbone on c_large and prints how far its logits of a PREFIX (the uncached sampler's input) are from the same rows of the full-length forward, and
whether its cached path (one token at start_pos = p) runs and agrees - see DESIGN.md §4b for the result.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from oracle import make_golden as MG  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.cases import CASES  # noqa: E402
import make_golden_ar as MGA  # noqa: E402

BOS = 3
RUNS = {"uncond": dict(cond=False, cfg=None), "cond": dict(cond=True, cfg=None), "cfg": dict(cond=True, cfg=1.5)}


def build_ar_reference(case):
    orig = MG._ref_cfg
    MG._ref_cfg = lambda c: MGA._ar_cfg(orig(c))
    try:
        d = MG.build_reference(case, torch.float32)
    finally:
        MG._ref_cfg = orig
    d.parameterization = "ar"
    d.backbone.eval()
    d.tokenizer = ref_shim.Cfg(bos_token_id=BOS)
    d.accelerator = ref_shim.Cfg(unwrap_model=lambda m: m)
    return d


def run_sampler(d, case, spec, use_kv_cache, noise=None):
    C = ref_shim.Cfg
    d.config.model.use_kv_cache = use_kv_cache
    d.use_kv_cache = use_kv_cache
    d.backbone.use_kv_cache = use_kv_cache       # (read by the reference's DIT and Attention at construction: models/dit.py:552, :1114)
    for blk in d.backbone.blocks:
        blk.attention.use_kv_cache = use_kv_cache
    d.config.eval = C(cfg=spec["cfg"], force_cfg_value=True, split_cfg_batches=False) if spec["cfg"] is not None else C(cfg=None)
    batch = d.update_batch({k: v.clone() for k, v in MG.make_batch(case).items()})
    x0_data, modality = batch["input_ids"], batch["modality"]
    B, L = x0_data.shape
    x0 = x0_unmask = None
    if spec["cond"]:
        x0 = x0_data.clone()
        x0_unmask = torch.zeros(B, L, dtype=torch.bool)
        x0_unmask[:, : case["txt_length"]] = True
    rec = {"noise": None, "zs": []}
    g_sample = torch.distributions.Gumbel.sample
    t_argmax = torch.Tensor.argmax

    def gumbel_sample(self, shape=torch.Size()):
        out = g_sample(self, shape) if noise is None else noise.clone()
        rec["noise"] = out.clone()
        return out

    def argmax(self, *a, **k):
        if self.dim() == 2 and self.shape[-1] == d.vocab_size:
            rec["zs"].append(self.detach().float().clone())
        return t_argmax(self, *a, **k)

    torch.distributions.Gumbel.sample = gumbel_sample
    torch.Tensor.argmax = argmax
    try:
        with torch.no_grad():
            torch.manual_seed(1234)
            x, nfe = d._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=modality)
    finally:
        torch.distributions.Gumbel.sample = g_sample
        torch.Tensor.argmax = t_argmax
    z = torch.stack(rec["zs"], 1)                               # [B, L-1, V]: next + noise[:, i]
    assert z.shape[1] == L - 1, z.shape
    top2 = z.topk(2, -1).values
    out = dict(noise=rec["noise"], x=x, nfe=torch.tensor(nfe), next=z - rec["noise"], margin=top2[..., 0] - top2[..., 1], modality=modality,
               bos=torch.tensor(BOS))
    if x0 is not None:
        out.update(x0=x0, x0_unmask=x0_unmask)
    if spec["cfg"] is not None:
        out["cfg"] = torch.tensor(spec["cfg"])
    return out


def find_rope_2d_quirk():
    """The reference backbone on c_large (2-D rope): logits of the prefix x[:, :n] against rows [:n] of the full-length forward (causal model: equal if the
    rotary rows did not depend on the input length).  Returns {n: max abs difference on text rows, on image rows}."""
    case = CASES["c_large"]
    d = build_ar_reference(case)
    batch = d.update_batch({k: v.clone() for k, v in MG.make_batch(case).items()})
    x, mod = batch["input_ids"], batch["modality"]
    L = x.shape[1]
    res = {}
    with torch.no_grad():
        full = d.backbone(x, None, modality=mod).float()
        for n in (L - 8, L - 1):
            pre = d.backbone(x[:, :n], None, modality=mod[:, :n]).float()
            txt = (mod[:, :n] == 0)
            diff = (pre - full[:, :n]).abs().amax(-1)
            res[n] = (float(diff[txt].max()), float(diff[~txt].max()) if (~txt).any() else 0.0)
        # the cached path: prefill position 0, then one token per step at start_pos = p
        d.backbone.use_kv_cache = True
        for blk in d.backbone.blocks:
            blk.attention.use_kv_cache = True
        B = x.shape[0]
        d.backbone.reset_kv_cache(batch_size=B, seq_len=L, dtype=torch.float32, device=torch.device("cpu"))
        try:
            rows = [d.backbone(x[:, p:p + 1], None, modality=mod[:, p:p + 1], start_pos=p).float() for p in range(L)]
            diff = (torch.cat(rows, 1) - full).abs().amax(-1)
            res["cached"] = (float(diff[mod == 0].max()), float(diff[mod != 0].max()))
        except RuntimeError as e:   # (its one-row table sliced again at start_pos > 0 is empty)
            res["cached"] = f"fails at the first step past position 0: {str(e).splitlines()[0]}"
    return res


def main():
    case = CASES["b_small"]
    d = build_ar_reference(case)
    for name, spec in RUNS.items():
        ref = run_sampler(d, case, spec, use_kv_cache=False)
        cached = run_sampler(d, case, spec, use_kv_cache=True, noise=ref["noise"])
        agree = bool(torch.equal(ref["x"], cached["x"]))
        out = {f"meta/{k}": np.array(v) for k, v in (("base_case", "b_small"), ("run", name), ("kv_cache_agrees", agree))}
        for k, v in ref.items():
            out[k] = MG._np(v)
        path = os.path.join(MG.GOLDEN_DIR, f"ar_sampler_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: nfe={int(ref['nfe'])} kv_cache_agrees={agree} min margin={float(ref['margin'].min()):.3g} -> {path} "
              f"({os.path.getsize(path) / 1024:.0f} KiB)")
    for n, r in find_rope_2d_quirk().items():
        if n == "cached":
            print(f"2-D rope, c_large: the cached path (start_pos = p, one token) vs the full-length forward: {r}")
        else:
            print(f"2-D rope, c_large: prefix of {n} tokens vs the full-length forward: max |d logits| text rows {r[0]:.3g}, image rows {r[1]:.3g}")


if __name__ == "__main__":
    main()
