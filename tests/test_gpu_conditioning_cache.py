"""eval.conditioning_cache on the GPU, on the `c_large` product in eval mode: after one build forward, conditional sampling runs the backbone on the generated
slice alone and attends to [cached conditioning keys ; fresh keys] through udm_attention_fwd_kv_split.

The identity (tests/test_conditioning_cache_host.py has it to the bit on kernel doubles): a "read" step equals the generated rows of the full-length forward under
the ModalityMask that blinds the given modality's queries to the other modality, on [given ; current slice] - in the unconditional half of guided sampling on
[[MASK] ... ; current slice].  Bound: relative L2 error per logits row < modality_cache_utils.ROW_BOUND = 1e-2, the project's bound for exactly this comparison
(two bf16 evaluation orders of one function); the achieved values go to the parity ledger."""
import pytest
import torch

import conditioning_cache_utils as U
import ledger
from modality_cache_utils import ROW_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "test_gpu_conditioning_cache"
B = 2


def _sigma(diff, t, rows):
    return diff._process_sigma(diff.noise(t * torch.ones(rows, device=DEV))[0])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("given", ["text", "image"])
def test_read_step_equals_generated_rows_of_masked_full_forward(given, guided):
    g, diff = U.cond_product(DEV)
    bb = diff.backbone
    x0, unmask, mod, sl = U.conditioning(g, diff, B, given, inpaint=True, device=DEV)
    L, Lt, V = x0.shape[1], g.case["txt_length"], diff.vocab_size
    Vt = g.case["text_vocab_size"]
    x = torch.where(unmask, x0, torch.full_like(x0, diff.mask_index))
    R = 2 * B if guided else B
    x_all, mod_all = (torch.cat([x, torch.full_like(x, diff.mask_index)], 0), torch.cat([mod, mod], 0)) if guided else (x, mod)
    plan_of = (lambda xr: torch.cat([xr[:B], xr[:B]], 0)) if guided else (lambda xr: None)
    cut = lambda t: None if t is None else t[:, sl].contiguous()      # noqa: E731
    sig = _sigma(diff, 0.7, R)
    mask = U.build_mask(R, Lt, given, DEV)
    tag0 = f"{given} given/{'guided' if guided else 'unguided'}"

    def check(x_rows, tag):
        read = bb.forward_masked_logits(cut(x_rows), sig, plan_ids=cut(plan_of(x_rows)), conditioning_cache="read")
        full = bb.forward_masked_logits(x_rows, sig, modality=mod_all, plan_ids=plan_of(x_rows), block_mask=mask)
        got, rows = U.slice_rows(read, V)
        ref, key = U.slice_rows_of_full(full, L, sl, V)
        assert torch.equal(rows, key) and key.numel() > 0
        ledger.check(TEST, f"{tag0}/{tag}: worst row rel_err", U.worst_row_rel_err(got, ref), ROW_BOUND)
        return ref, rows

    with torch.no_grad():
        bb.set_conditioning_cache(B, L, DEV, given=given, guided=guided)
        bb.forward_masked_logits(x_all, sig, modality=mod_all, plan_ids=plan_of(x_all), conditioning_cache="build")
        check(x_all, "a/read step vs generated rows of the masked full forward")
        # the slice changes, the cache is not rebuilt
        x2 = x_all.clone()
        masked = (x2[:B] == diff.mask_index).nonzero()
        for b, l in masked[::2].tolist():
            x2[b, l] = (7 * b + 3 * l) % (diff.mask_index - 1) if l < Lt else Vt + (7 * b + 3 * l) % (V - Vt)
        assert (x2[:B] == diff.mask_index).any() and not torch.equal(x2, x_all)
        if guided:
            x2[B:, sl] = torch.where(unmask[:, sl], torch.full_like(x2[:B, sl], diff.mask_index), x2[:B, sl])
        ref2, rows2 = check(x2, "b/after the slice changed, cache not rebuilt")
        if guided:      # eval.split_cfg_batches: each half through a batch-offset view of the cache
            n = rows2.numel() // 2
            for half in (0, 1):
                one = bb.forward_masked_logits(cut(x2[half * B:(half + 1) * B]), sig[:B], plan_ids=cut(x2[:B]), conditioning_cache="read", cache_row0=half * B)
                got_h, rows_h = U.slice_rows(one, V)
                assert torch.equal(rows_h, rows2[:n])
                ledger.check(TEST, f"{tag0}/c/half {half} alone (batch-offset cache view): worst row rel_err", U.worst_row_rel_err(got_h, ref2[half * n:(half + 1) * n]),
                             ROW_BOUND)
        # the slice alone, without the cache, gives other logits: the cache is read
        alone, rows3 = U.slice_rows(bb.forward_masked_logits(cut(x2), sig, modality=cut(mod_all), plan_ids=cut(plan_of(x2))), V)
        assert torch.equal(rows3, rows2)
        err = U.worst_row_rel_err(alone, ref2)
        ledger.record(TEST, f"{tag0}/d/slice-only forward without the cache: worst row rel_err (must EXCEED the bound)", err, ROW_BOUND)
        assert err > ROW_BOUND, err
        bb.reset_kv_cache()
    assert bb._cc is None


@pytest.mark.parametrize("given,cfg,split,inpaint", [("text", None, False, False), ("image", 2.0, False, True), ("text", 2.0, True, False)],
                         ids=["text-given", "image-given-cfg-inpaint", "text-given-cfg-split"])
@pytest.mark.parametrize("predictor", U.PREDICTORS)
def test_sample_with_the_key(predictor, given, cfg, split, inpaint):
    """No [MASK] left, the given tokens kept, deterministic for a seed, the cache dropped, nfe as in the key-off run.  maskgit / first_hitting evaluate once per
    step whatever is drawn; ddpm_cache skips the evaluation after a step that left x unchanged, so its count follows the draws (and the key changes the logits
    they are made from): it runs 2 steps, in which a [MASK] token survives step 0 with probability 1 / 2 and step 1 never - all [MASK] tokens of both rows
    surviving has probability < 2^-16, so both runs evaluate in every step."""
    steps = 2 if predictor == "ddpm_cache" else 5
    g, on = U.cond_product(DEV, True, cfg=cfg, split=split)
    x0, unmask, mod, sl = U.conditioning(g, on, B, given, inpaint=inpaint, device=DEV)
    kw = dict(num_steps=steps, x0=x0, x0_unmask=unmask, modality=mod, seed=5, predictor=predictor, return_nfe=True)
    a, nfe_on = on.sample(**kw)
    b, _ = on.sample(**kw)
    assert torch.equal(a, b) and a.shape == x0.shape
    assert not (a == on.mask_index).any() and torch.equal(a[unmask], x0[unmask])
    Vt = g.case["text_vocab_size"]
    Lt = g.case["txt_length"]
    assert bool((a[:, :Lt] < Vt).all()) and bool((a[:, Lt:] >= Vt).all())                     # every slice holds ids of its modality
    assert on.sample_step_modes == ["build"] + ["slice"] * (steps - 1)
    assert on.backbone._cc is None and on._cond is None
    g, off = U.cond_product(DEV, False, cfg=cfg, split=split)
    _, nfe_off = off.sample(**kw)
    assert nfe_on == nfe_off == steps + 1, (nfe_on, nfe_off)
