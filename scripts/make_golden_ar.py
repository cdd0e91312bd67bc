"""Golden vectors of the AR baseline (parameterization=ar, trainer.ar_shift, model.full_attention=false; configs/experiments/ar.yaml) from the IMPORTED
reference, CPU fp32 ("truth") and CPU bf16 autocast (the reference's own bf16 floor).  Build container only (the reference does not travel):

    python scripts/make_golden_ar.py            # writes tests/golden/ar_b_small.npz, tests/golden/ar_c_large.npz

TEST INFRASTRUCTURE.  The geometries are those of oracle/cases.py `b_small` / `c_large` (same parameters, same batch), with the ar overrides applied to
the config tree oracle/make_golden.py builds.  Under AR the reference draws no t and corrupts nothing (model.py:840-918), so the cases'
`mask_entire_modality` and `softmin_snr` have no effect; the fixture lists them under meta/unused.  b_small covers the padded masked mean
(ragged_text, force_full_attention_mask_loss_only), c_large the text / image-weighted loss.

Recorded: the batch, the parameters, the logits [B, L, V] the backbone returns, the AR log-probs [B, L-1, V] after the shift / masking / log-softmax
(model.py:717-781), the per-token log p of the targets x0[:, 1:], the loss and every parameter gradient (fp32 run; of the bf16 run its per-parameter
rel-RMS distance from the fp32 gradient).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from oracle.cases import CASES  # noqa: E402

AR_CASES = {"ar_b_small": "b_small", "ar_c_large": "c_large"}
UNUSED = ("mask_entire_modality", "softmin_snr")


def _ar_cfg(cfg):
    cfg.parameterization = "ar"
    cfg.trainer.ar_shift = True
    cfg.trainer.rand_ar_modality_dropout = None
    cfg.model.full_attention = False
    return cfg


def run_reference_ar(case, dtype):
    orig = MG._ref_cfg
    MG._ref_cfg = lambda c: _ar_cfg(orig(c))   # the reference's DIT reads model.full_attention when it is built (models/dit.py:1118)
    try:
        d = MG.build_reference(case, dtype)
    finally:
        MG._ref_cfg = orig
    d.parameterization = "ar"
    rec = {}
    hook = d.backbone.register_forward_hook(lambda mod, args, out: rec.__setitem__("logits", out.detach().float().clone()))
    orig_forward = d.forward

    def forward(*a, **k):
        out = orig_forward(*a, **k)
        lp = out[0] if isinstance(out, tuple) else out
        rec["log_probs"] = lp.detach().float().clone()
        return out

    d.forward = forward
    batch = MG.make_batch(case)
    torch.manual_seed(case["step_seed"])
    upd = d.update_batch({k: v.clone() for k, v in batch.items()})
    out = d.compute_loss(upd, "train", 1)
    out.loss.backward()
    hook.remove()
    x0 = upd["input_ids"]
    rec["log_p"] = rec["log_probs"].gather(-1, x0[:, 1:, None])[..., 0]
    rec.update(input_ids=x0, attention_mask=upd["attention_mask"], modality=upd["modality"], loss=out.loss.detach(), nlls=out.nlls.detach(),
               token_mask=out.token_mask)
    for k in ("txt_loss", "img_loss"):
        v = getattr(out, k)
        if torch.is_tensor(v):
            rec[k] = v.detach()
    grads = {n: p.grad.detach().clone() for n, p in d.backbone.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in d.backbone.named_parameters()}
    return batch, rec, params, grads


def main(names=None):
    for name, base in AR_CASES.items():
        if names and name not in names:
            continue
        case = CASES[base]
        out = {"meta/base_case": np.array(base), "meta/unused": np.array(list(UNUSED))}
        batch, rec32, params, grads32 = run_reference_ar(case, torch.float32)
        _, rec16, params16, grads16 = run_reference_ar(case, torch.bfloat16)
        for n in params:
            assert torch.equal(params[n], params16[n]), n
        for k, v in batch.items():
            out["batch/" + k] = MG._np(v)
        for k, v in params.items():
            out["param/" + k] = MG._np(v)
        for tag, rec in (("fp32", rec32), ("bf16", rec16)):
            for k, v in rec.items():
                if tag == "bf16" and k == "log_probs":   # (not read: the floors below are taken on logits and log p)
                    continue
                out[f"{tag}/{k}"] = MG._np(v)
        for k, v in grads32.items():
            out[f"fp32/grad/{k}"] = MG._np(v)
        # the bf16 run's gradients enter the tests only as their distance from the fp32 ones (rel-RMS per parameter): stored as that number, which keeps
        # the fixture under the size limit for a committed file
        for k, v in grads16.items():
            g32 = grads32[k].double()
            out[f"bf16/grad_relrms/{k}"] = np.array(float((v.double() - g32).norm() / g32.norm().clamp_min(1e-30)))
        path = os.path.join(MG.GOLDEN_DIR, f"{name}.npz")
        np.savez_compressed(path, **out)
        l32, l16 = float(out["fp32/loss"]), float(out["bf16/loss"])
        print(f"{name}: loss fp32={l32:.6f} bf16={l16:.6f} rel={abs(l16 - l32) / abs(l32):.2e} -> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
