"""eval.attention_caching_read_cache on the GPU, on the `c_large` product in eval mode: the text steps of the attention-caching sampler attend to
[fresh text keys ; cached image keys] through udm_attention_fwd_kv.

The identity (tests/test_modality_cache_host.py has it on kernel doubles): a read-cache text step equals the text rows of a full-length forward under
ModalityMask(txt_drop = 0, img_drop = 1) on [current text ; image tokens that entered the build step].  Bound: relative L2 error per logits row < 1e-2, what
tests/test_gpu_ar_sampler.py holds KV-cached decode rows to against the full forward; the achieved values go to the parity ledger."""
import warnings

import pytest
import torch

import ledger
import modality_cache_utils as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "test_gpu_modality_cache"


def _sigma(diff, s, i, B):
    return diff._process_sigma(diff.noise(s["timesteps"][i].to(DEV) * torch.ones(B, device=DEV))[0])


def _check_read_step(diff, x_text, x_img, mod, sig, tag):
    """the read-cache text step on x_text against the text rows of the masked full-length forward on [x_text ; x_img]; returns (read rows, reference rows)"""
    bb = diff.backbone
    B, Lt = x_text.shape
    L, V = Lt + x_img.shape[1], diff.vocab_size
    read = bb.forward_masked_logits(x_text.contiguous(), sig, modality=mod[:, :Lt].contiguous(), modality_cache="read")
    full = bb.forward_masked_logits(torch.cat([x_text, x_img], 1), sig, modality=mod, block_mask=U.build_mask(B, Lt, DEV))
    got, rows = U.text_rows(read, V)
    ref, key = U.text_rows_of_full(full, L, Lt, V)
    assert torch.equal(rows, key)
    if key.numel():
        ledger.check(TEST, tag, U.worst_row_rel_err(got, ref), U.ROW_BOUND)
    return got, ref


def test_read_cache_text_step_equals_text_rows_of_masked_full_forward():
    g, s, diff = U.caching_product(DEV, True)
    bb = diff.backbone
    B, L = s["x_init"].shape
    Lt, V = g.case["txt_length"], diff.vocab_size
    mod = s["modality"].to(DEV)
    x_build = s["step1/x"].to(DEV)
    sig = _sigma(diff, s, 1, B)
    with torch.no_grad():
        bb.set_flex_attention_cache(B, L, DEV, None, read_cache=True)
        bb.forward_masked_logits(x_build, sig, modality=mod, block_mask=U.build_mask(B, Lt, DEV), modality_cache="build")
        x_img = x_build[:, Lt:].contiguous()
        # (a) right after the build step
        x_text = x_build[:, :Lt].contiguous()
        assert (x_text == diff.mask_index).any()
        _check_read_step(diff, x_text, x_img, mod, sig, "a/read-cache text step vs text rows of the masked full forward: worst row rel_err")
        # (b) after unmasking some text tokens, the cache not rebuilt
        x_text2 = x_text.clone()
        masked = (x_text2 == diff.mask_index).nonzero()
        for b, l in masked[::2].tolist():
            x_text2[b, l] = (7 * b + 3 * l) % (diff.mask_index - 1)
        assert (x_text2 == diff.mask_index).any() and not torch.equal(x_text2, x_text)
        got2, ref2 = _check_read_step(diff, x_text2, x_img, mod, sig, "b/after unmasking text tokens, cache not rebuilt: worst row rel_err")
        # (c) the text-only path (key false: text queries on text keys alone) gives other logits: the cache is read
        alone, _ = U.text_rows(bb.forward_masked_logits(x_text2, sig, modality=mod[:, :Lt].contiguous()), V)
        err_c = U.worst_row_rel_err(alone, ref2)
        ledger.record(TEST, "c/text-only step vs text rows of the masked full forward: worst row rel_err (must EXCEED the bound)", err_c, U.ROW_BOUND)
        assert err_c > U.ROW_BOUND, err_c
        bb.reset_kv_cache()
    assert bb._mc is None


def test_sample_with_read_cache():
    g, s, off = U.caching_product(DEV, False)
    steps = int(s["steps"])
    B, L = s["x_init"].shape
    Lt = g.case["txt_length"]
    mod = s["modality"].to(DEV)
    off.sample(num_steps=steps, batch_size=B, modality=mod, seed=5)
    modes_off = list(off.sample_step_modes)
    g, s, on = U.caching_product(DEV, True)
    a = on.sample(num_steps=steps, batch_size=B, modality=mod, seed=5)
    b = on.sample(num_steps=steps, batch_size=B, modality=mod, seed=5)
    assert torch.equal(a, b) and not (a == on.mask_index).any() and a.shape == (B, L)      # deterministic for a fixed seed, no [MASK] left
    assert on.sample_step_modes == modes_off and {"full", "build", "text"} <= set(modes_off)
    assert on.backbone._mc is None                                                          # freed

    # every text step's logits against [that step's text ; the image tokens that entered the last build step]
    bb = on.backbone
    seen, state = [], dict(x_build=None)
    upd, fwd = on._ddpm_caching_update, bb.forward_masked_logits

    def spy_fwd(xt, sigma=None, **kw):
        out = fwd(xt, sigma, **kw)
        if kw.get("modality_cache") == "build":
            state["x_build"] = xt.clone()
        elif kw.get("modality_cache") == "read":
            seen.append((xt.clone(), sigma, state["x_build"][:, Lt:].clone(), tuple(t.clone() if torch.is_tensor(t) else t for t in out)))
        return out

    bb.forward_masked_logits = spy_fwd
    x_steps = []
    on._ddpm_caching_update = lambda x, t, dt, **kw: (x_steps.append(tuple(x.shape)), upd(x, t, dt, **kw))[1]
    c = on.sample(num_steps=steps, batch_size=B, modality=mod, seed=5)
    bb.forward_masked_logits = fwd
    assert torch.equal(c, a)
    assert [sh == (B, Lt) for sh in x_steps] == [m == "text" for m in modes_off]
    assert seen, "no text step ran its forward"
    V = on.vocab_size
    with torch.no_grad():
        for j, (x_text, sig, x_img, out) in enumerate(seen):
            full = fwd(torch.cat([x_text, x_img], 1), sig, modality=mod, block_mask=U.build_mask(B, Lt, DEV))
            got, rows = U.text_rows(out, V)
            ref, key = U.text_rows_of_full(full, L, Lt, V)
            assert torch.equal(rows, key)
            if key.numel():
                ledger.check(TEST, f"d/sample() text-step forward {j}: worst row rel_err vs the masked full forward", U.worst_row_rel_err(got, ref), U.ROW_BOUND)


def _syncs(fn):
    """number of synchronising calls torch reports in fn() (sync debug mode "warn")"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def test_read_cache_text_step_adds_no_host_sync():
    """The sampler's step reads the number of [MASK] rows back (the head runs on those rows): the key-false text step does not pass sync mode "error" as a
    whole.  So the baseline is measured - the synchronising calls of one key-false text-step forward - and the read-cache forward is held to no more."""
    g, s, diff = U.caching_product(DEV, True)
    bb = diff.backbone
    B, L = s["x_init"].shape
    Lt = g.case["txt_length"]
    mod = s["modality"].to(DEV)
    x_build = s["step1/x"].to(DEV)
    sig = _sigma(diff, s, 1, B)
    x_text, mod_text = x_build[:, :Lt].contiguous(), mod[:, :Lt].contiguous()
    with torch.no_grad():
        bb.set_flex_attention_cache(B, L, DEV, None, read_cache=True)
        bb.forward_masked_logits(x_build, sig, modality=mod, block_mask=U.build_mask(B, Lt, DEV), modality_cache="build")
        for _ in range(2):   # (warm: first-use allocations and attribute calls are not the step's)
            bb.forward_masked_logits(x_text, sig, modality=mod_text)
            bb.forward_masked_logits(x_text, sig, modality=mod_text, modality_cache="read")
        base = _syncs(lambda: bb.forward_masked_logits(x_text, sig, modality=mod_text))
        new = _syncs(lambda: bb.forward_masked_logits(x_text, sig, modality=mod_text, modality_cache="read"))
        bb.reset_kv_cache()
    ledger.record(TEST, "e/synchronising calls of a key-false text-step forward", base)
    ledger.record(TEST, "e/synchronising calls of a read-cache text-step forward", new, base)
    assert new <= base, (new, base)
