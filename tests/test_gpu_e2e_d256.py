"""One training step at head dim 256 against the CPU oracle: the body of test_training_step_matches_oracle_at_full_width (tests/test_gpu_fullwidth_oracle.py) -
the same seeded batch, rng_device = "cpu", the oracle's fp32 pass as the truth and its `bf16=True, flash_rounding=True` pass as the floor.

  d256_2blocks_b2      hidden 512, 2 heads, 2 blocks: D = 256 attention and the narrow-row qk-norm + rope kernel, block -> block composition
  xxl_width_1block_b2  hidden 4096, 16 heads, 1 block: the xxl width - the d = 4096 row kernels and the K = 4096 / 16 384 GEMMs with D = 256 attention in between

Asserted: xt, move_indices, token_mask, t bit-exact; loss relative error <= 1e-3 and NLL rel-RMS <= 4.5e-3 against the fp32 oracle (LOSS_BOUND, NLL_BOUND of
tests/test_gpu_e2e.py); gradients by the floor rule of the full-width test: the worst parameter <= 1.5 x the floor's worst parameter, every parameter <= 2 x its
own floor.  The achieved values go into the parity ledger."""
import json
import os

import pytest
import torch

from ledger import check, record
from oracle import unidisc_oracle as O
from oracle.cases import lumina_rope_2d
from product_utils import product_config
from test_gpu_fullwidth_oracle import _LARGE, _make_batch, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_BOUND, NLL_BOUND = 1e-3, 4.5e-3

_D256 = dict(_LARGE, linear_factor=1.0, txt_length=64, img_length=256, text_vocab_size=1001, vocab_size=1001 + 512)
CASES_D256 = {
    "d256_2blocks_b2": (dict(_D256, hidden_size=512, n_heads=2, n_blocks=2), 2),
    "xxl_width_1block_b2": (dict(_D256, hidden_size=4096, n_heads=16, n_blocks=1), 2),
}


@pytest.mark.parametrize("name", sorted(CASES_D256))
def test_training_step_matches_oracle_at_head_dim_256(name):
    case, B = CASES_D256[name]
    from unidisc_amd import Diffusion

    assert case["hidden_size"] // case["n_heads"] == 256
    cfg = product_config(case)
    torch.manual_seed(0)
    diff = Diffusion(cfg, None, DEV)
    diff.backbone.train()
    diff.rng_device = "cpu"
    wg = torch.Generator().manual_seed(5)
    with torch.no_grad():   # non-trivial head weights (the reference zero-initialises them)
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "adaLN_modulation" in n:
                p.copy_((torch.randn(p.shape, generator=wg) * (0.5 / p.shape[-1] ** 0.5)).to(DEV))
    assert diff.vocab_size == case["vocab_size"] and diff.mask_index == case["text_vocab_size"] - 1
    P = {k: v.detach().cpu().clone().requires_grad_() for k, v in diff.backbone.named_parameters()}
    batch = _make_batch(case, B, torch.Generator().manual_seed(77))

    ocfg = O.OracleConfig.from_case(case)
    bufs = O.make_buffers(ocfg, lumina_rope_2d)
    ob = O.update_batch(ocfg, {k: v.clone() for k, v in batch.items()})
    o32 = O.compute_loss(ocfg, P, bufs, ob, torch.Generator().manual_seed(123))
    o32.loss.backward()
    P16f = {k: v.detach().clone().requires_grad_() for k, v in P.items()}
    o16 = O.compute_loss(ocfg, P16f, bufs, ob, torch.Generator().manual_seed(123), bf16=True, flash_rounding=True)
    o16.loss.backward()

    torch.manual_seed(123)
    out = diff.training_step({k: v.clone() for k, v in batch.items()}, 1)
    assert torch.equal(diff._last["xt"].cpu(), o32.aux["xt"])
    assert torch.equal(diff._last["move_indices"].cpu(), o32.aux["move_indices"])
    assert torch.equal(out.token_mask.cpu(), o32.token_mask)
    assert torch.equal(diff._last["t"].cpu(), o32.aux["t"])
    assert 0 < int(o32.aux["move_indices"].sum()) < o32.aux["move_indices"].numel()

    l, l32, l16 = float(out.loss.detach()), float(o32.loss.detach()), float(o16.loss.detach())
    record(name, "ref_bf16_vs_fp32_loss_rel", abs(l16 - l32) / abs(l32), note="the reference's own bf16-vs-fp32 noise floor (oracle bf16 emulation)")
    check(name, "loss_rel_vs_fp32_oracle", abs(l - l32) / abs(l32), LOSS_BOUND)
    record(name, "ref_bf16_vs_fp32_nll_relrms", _rel(o16.nlls.detach(), o32.nlls))
    check(name, "nll_relrms_vs_fp32_oracle", _rel(out.nlls.cpu(), o32.nlls), NLL_BOUND)
    assert torch.all(out.nlls.cpu()[~o32.aux["move_indices"]] == 0)   # unmasked tokens: nll exactly 0

    out.loss.backward()
    torch.cuda.synchronize()
    errs = []
    for k, p in diff.backbone.named_parameters():
        if P[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        errs.append((_rel(p.grad.cpu(), P[k].grad), k))
    errs.sort(reverse=True)
    floor_f = {k: _rel(P16f[k].grad, P[k].grad) for k in P if P[k].grad is not None}
    ff = sorted(((v, k) for k, v in floor_f.items()), reverse=True)
    record(name, "ref_bf16_flash_rounding_vs_fp32_grad_relrms_worst_param", ff[0][0], note=ff[0][1])
    record(name, "ref_bf16_flash_rounding_vs_fp32_grad_relrms_median_param", ff[len(ff) // 2][0])
    ratios = sorted(((e / max(floor_f[k], 1e-12), k) for e, k in errs), reverse=True)
    if os.environ.get("UDM_DUMP_GRAD_ERRS"):   # per-parameter table (ours, flash-rounding floor) for diagnosis
        with open(os.environ["UDM_DUMP_GRAD_ERRS"] + f".{name}.json", "w") as f:
            json.dump({k: dict(ours=e, floor_flash=floor_f[k], numel=P[k].numel(), gnorm=float(P[k].grad.norm())) for e, k in errs}, f, indent=0)
    record(name, "grad_relrms_worst_param", errs[0][0], note=errs[0][1])
    record(name, "grad_relrms_median_param", errs[len(errs) // 2][0])
    record(name, "grad_err_over_flash_rounding_floor_median_ratio", ratios[len(ratios) // 2][0])
    faults = []
    for key, got, bound, note in (("grad_relrms_worst_param_over_flash_rounding_floor_worst", errs[0][0] / ff[0][0], 1.5, f"{errs[0][1]} vs {ff[0][1]}"),
                                  ("grad_err_over_flash_rounding_floor_worst_ratio", ratios[0][0], 2.0, ratios[0][1])):
        try:
            check(name, key, got, bound, note=note)
        except AssertionError as e:
            faults.append(f"{e} [{note}]")
    assert not faults, "\n".join(faults)
