"""eval.conditioning_cache on the CPU with kernel doubles (tests/fake_kernels_cond.py): the host logic of the conditioning K / V cache on the `c_large` case
(d = 64, H = 2, D = 32, L = 16 + 16, 2-D rope, modality embedding).

The identity under test: under the ModalityMask that blinds the GIVEN modality's queries to the other modality, the given rows' K / V depend on the given
tokens alone, so a "read" step on the generated slice equals - on the doubles to the bit - the generated rows of the masked full-length forward on
[given ; current slice]; in the unconditional half of guided sampling the given slice is all [MASK].  A whole seeded sample() with the key on therefore returns
the tokens of a reference loop that runs that masked full-length forward at every step (conditioning_cache_utils.reference_backbone)."""
import pytest
import torch

import conditioning_cache_utils as U
import fake_kernels_cond

B = 2
STEPS = 6


@pytest.fixture
def doubles(monkeypatch):
    from unidisc_amd import diffusion as diff_mod, dit as dit_mod

    monkeypatch.setattr(dit_mod, "K", fake_kernels_cond)
    monkeypatch.setattr(diff_mod, "K", fake_kernels_cond)
    fake_kernels_cond.CALLS.clear()
    return fake_kernels_cond


def _sigma(diff, t, rows):
    return diff._process_sigma(diff.noise(t * torch.ones(rows))[0])


def _unmask_some(diff, x, g, sl):
    """a few [MASK] positions of the generated slice take tokens of their modality"""
    x = x.clone()
    Vt, V = g.case["text_vocab_size"], g.case["vocab_size"]
    masked = (x == diff.mask_index).nonzero()
    for b, l in masked[::2].tolist():
        x[b, l] = (7 * b + 3 * l) % (diff.mask_index - 1) if sl.start == 0 else Vt + (7 * b + 3 * l) % (V - Vt)
    assert (x == diff.mask_index).any()
    return x


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("given", ["text", "image"])
def test_read_step_is_the_generated_rows_of_the_masked_full_forward(doubles, given, guided):
    g, diff = U.cond_product("cpu")
    bb = diff.backbone
    x0, unmask, mod, sl = U.conditioning(g, diff, B, given, inpaint=True)
    L, Lt, V = x0.shape[1], g.case["txt_length"], diff.vocab_size
    Lq = sl.stop - sl.start
    x = torch.where(unmask, x0, torch.full_like(x0, diff.mask_index))
    R = 2 * B if guided else B
    if guided:      # [x ; x with everything given masked]: one batch, the same positions from both halves
        x_all, plan, mod_all = torch.cat([x, torch.full_like(x, diff.mask_index)], 0), torch.cat([x, x], 0), torch.cat([mod, mod], 0)
    else:
        x_all, plan, mod_all = x, None, mod
    sig = _sigma(diff, 0.7, R)
    mask = U.build_mask(R, Lt, given, "cpu")

    with pytest.raises(RuntimeError, match="no conditioning cache"):
        bb.forward_masked_logits(x_all, sig, modality=mod_all, plan_ids=plan, conditioning_cache="build")
    bb.set_conditioning_cache(B, L, "cpu", given=given, guided=guided)
    cc = bb._cc
    assert len(cc.K) == len(cc.V) == g.case["n_blocks"] and all(k.shape == (R, L, g.case["hidden_size"]) and k.dtype == torch.bfloat16 for k in cc.K + cc.V)
    with pytest.raises(RuntimeError, match="no conditioning keys"):
        bb.forward_masked_logits(x_all[:, sl].contiguous(), sig, plan_ids=None if plan is None else plan[:, sl].contiguous(), conditioning_cache="read")
    built = bb.forward_masked_logits(x_all, sig, modality=mod_all, plan_ids=plan, conditioning_cache="build")
    plain = bb.forward_masked_logits(x_all, sig, modality=mod_all, plan_ids=plan, block_mask=mask)
    assert built[2] == plain[2] and torch.equal(built[1], plain[1]) and torch.equal(built[0][:built[2], :V], plain[0][:built[2], :V])      # the build step IS that forward
    assert all(bool((k.float().abs().sum(-1) > 0).all()) for k in cc.K + cc.V)
    gsl = slice(0, Lt) if given == "text" else slice(Lt, L)
    given_before = [k[:, gsl].clone() for k in cc.K + cc.V]

    def check(x_slices, tag):
        xs, ps = x_slices[:, sl].contiguous(), (None if plan is None else plan_of(x_slices)[:, sl].contiguous())
        fake_kernels_cond.CALLS.clear()
        read = bb.forward_masked_logits(xs, sig, plan_ids=ps, conditioning_cache="read")
        assert fake_kernels_cond.CALLS == [(R, Lq, L, (R, L, g.case["hidden_size"]), True)] * g.case["n_blocks"]      # the slice's queries, all L slots
        full = bb.forward_masked_logits(x_slices, sig, modality=mod_all, plan_ids=None if plan is None else plan_of(x_slices), block_mask=mask)
        got, rows = U.slice_rows(read, V)
        ref, key = U.slice_rows_of_full(full, L, sl, V)
        assert torch.equal(rows, key) and key.numel() > 0, tag
        assert torch.equal(got, ref), (tag, U.worst_row_rel_err(got, ref))
        return got, rows

    def plan_of(x_rows):      # both halves report the [MASK] positions of the conditional half
        return torch.cat([x_rows[:B], x_rows[:B]], 0)

    check(x_all, "right after the build step")
    # the slice changes, the cache is not rebuilt: the given slots are only read
    x2 = x_all.clone()
    x2[:B] = _unmask_some(diff, x_all[:B], g, sl)
    if guided:
        x2[B:, sl] = torch.where(unmask[:, sl], torch.full_like(x2[:B, sl], diff.mask_index), x2[:B, sl])
    got2, rows2 = check(x2, "after the slice changed")
    for t, before in zip(cc.K + cc.V, given_before):
        assert torch.equal(t[:, gsl], before)
    # ... and without the cache the slice alone gives other logits: the cache is read
    alone = bb.forward_masked_logits(x2[:, sl].contiguous(), sig, modality=mod_all[:, sl].contiguous(), plan_ids=None if plan is None else plan_of(x2)[:, sl].contiguous())
    got3, rows3 = U.slice_rows(alone, V)
    assert torch.equal(rows3, rows2) and U.worst_row_rel_err(got3, got2) > 1e-2
    if guided:      # eval.split_cfg_batches: each half alone, through a batch-offset view of the cache, gives the rows of the one-batch pass
        n = rows2.numel() // 2
        for half in (0, 1):
            one = bb.forward_masked_logits(x2[half * B:(half + 1) * B, sl].contiguous(), sig[:B], plan_ids=x2[:B, sl].contiguous(), conditioning_cache="read",
                                           cache_row0=half * B)
            got_h, rows_h = U.slice_rows(one, V)
            assert torch.equal(rows_h, rows2[:n]) and torch.equal(got_h, got2[half * n:(half + 1) * n])
        with pytest.raises(ValueError, match="cache row"):
            bb.forward_masked_logits(x2[:B, sl].contiguous(), sig[:B], conditioning_cache="read", cache_row0=1)
    with pytest.raises(ValueError, match="two different caches"):
        bb.forward_masked_logits(x2[:, sl].contiguous(), sig, conditioning_cache="read", modality_cache="read")
    with pytest.raises(NotImplementedError, match="sample ids"):
        bb.forward_masked_logits(x2[:, sl].contiguous(), sig, conditioning_cache="read", sample_ids=torch.zeros(R, Lq, dtype=torch.int64))
    bb.reset_kv_cache()
    assert bb._cc is None


def _sample(diff, x0, unmask, mod, predictor, **kw):
    return diff.sample(num_steps=STEPS, x0=x0, x0_unmask=unmask, modality=mod, seed=11, predictor=predictor, return_nfe=True, **kw)


CASES = [(p, given, None, False, False) for p in U.PREDICTORS for given in ("text", "image")]
CASES += [(p, "text", 2.0, False, False) for p in U.PREDICTORS] + [("maskgit", "image", 2.0, False, False)]
CASES += [("maskgit", "text", 2.0, True, False), ("ddpm_cache", "image", 2.0, True, False)]                 # eval.split_cfg_batches
CASES += [("maskgit", "text", None, False, True), ("ddpm_cache", "image", 2.0, False, True), ("first_hitting", "text", 2.0, True, True)]      # inpainting


@pytest.mark.parametrize("predictor,given,cfg,split,inpaint", CASES)
def test_sample_returns_the_tokens_of_the_masked_full_length_loop(doubles, predictor, given, cfg, split, inpaint):
    g, on = U.cond_product("cpu", True, cfg=cfg, split=split)
    x0, unmask, mod, sl = U.conditioning(g, on, B, given, inpaint=inpaint)
    calls = []
    fwd = on.backbone.forward_masked_logits
    on.backbone.forward_masked_logits = lambda xt, *a, **kw: (calls.append((tuple(xt.shape), kw.get("conditioning_cache"), kw.get("cache_row0", 0))), fwd(xt, *a, **kw))[1]
    x_on, nfe_on = _sample(on, x0, unmask, mod, predictor)
    assert on.sample_step_modes == ["build"] + ["slice"] * (STEPS - 1)
    assert on.backbone._cc is None and on._cond is None                                   # dropped at the end
    assert not (x_on == on.mask_index).any() and torch.equal(x_on[unmask], x0[unmask])      # nothing left masked, the given tokens kept
    L, Lq, R = x0.shape[1], sl.stop - sl.start, (2 * B if cfg is not None else B)
    assert calls and calls[0][1] == "build" and all(c[1] == ("build" if c[0][1] == L else "read") for c in calls)
    passes = {B} if (cfg is None or split) else {B, R}      # (unguided passes of B rows: zero guidance weight at t = 1, the noise-removal forward)
    assert all(c[0][1] in (L, Lq) and c[0][0] in passes for c in calls) and sum(c[0][1] == L for c in calls) == (2 if (split and cfg is not None) else 1)
    assert {c[2] for c in calls} == ({0, B} if (split and cfg is not None) else {0})

    g, ref = U.cond_product("cpu", True, cfg=cfg, split=split)
    ref_calls = U.reference_backbone(ref, g, given, x0[:, slice(0, sl.start) if sl.start else slice(sl.stop, L)], B)
    x_ref, nfe_ref = _sample(ref, x0, unmask, mod, predictor)
    assert [c[:3] for c in ref_calls] == [(c[1], c[0], c[2]) for c in calls]
    assert torch.equal(x_on, x_ref) and nfe_on == nfe_ref

    # nfe counts as before.  maskgit / first_hitting: one evaluation per step whatever is drawn.  ddpm_cache: a step that leaves x unchanged keeps its logits and
    # the next one evaluates nothing, so the count follows the draws, and the key changes the logits they are made from; with 2 steps a [MASK] token survives
    # step 0 with probability 1 / 2 and no step 1, so both runs change x in every step (all of >= 8 tokens surviving: < 2^-8 per row) and count 2 + 1.
    g, off = U.cond_product("cpu", False, cfg=cfg, split=split)
    steps = 2 if predictor == "ddpm_cache" else STEPS
    if predictor == "ddpm_cache":
        nfe_on = on.sample(num_steps=steps, x0=x0, x0_unmask=unmask, modality=mod, seed=11, predictor=predictor, return_nfe=True)[1]
    x_off, nfe_off = off.sample(num_steps=steps, x0=x0, x0_unmask=unmask, modality=mod, seed=11, predictor=predictor, return_nfe=True)
    assert nfe_off == nfe_on == steps + 1 and off.sample_step_modes == [] and off.backbone._cc is None


def test_key_absent_or_false_is_the_path_as_it_was(doubles):
    x = []
    for key in (None, False):
        g, diff = U.cond_product("cpu", key, cfg=2.0)
        x0, unmask, mod, _ = U.conditioning(g, diff, B, "text")
        kinds = []
        fwd = diff.backbone.forward_masked_logits
        diff.backbone.forward_masked_logits = lambda *a, **kw: (kinds.append("conditioning_cache" in kw or "cache_row0" in kw), fwd(*a, **kw))[1]
        x.append(_sample(diff, x0, unmask, mod, "maskgit")[0])
        assert kinds and not any(kinds) and diff.backbone._cc is None and not fake_kernels_cond.CALLS
    assert torch.equal(x[0], x[1])


@pytest.mark.parametrize("what", ["no_x0", "neither", "both", "time_conditioning", "sample_ids", "ar", "attention_caching", "text_layout"])
def test_sampler_refusals(doubles, what):
    extra = dict(attention_caching=True, attention_caching_txt_to_img_ratio=3) if what == "attention_caching" else {}
    g, diff = U.cond_product("cpu", True, **extra)
    x0, unmask, mod, sl = U.conditioning(g, diff, B, "text")
    kw = dict(num_steps=STEPS, x0=x0, x0_unmask=unmask, modality=mod, predictor="ddpm_cache")
    match = "conditioning_cache"
    if what == "no_x0":
        kw.update(x0=None, x0_unmask=None, batch_size=B)
        match = "neither is"
    elif what == "neither":
        unmask[0, 0] = False
        match = "neither is"
    elif what == "both":
        unmask[:] = True
        match = "both are"
    elif what == "time_conditioning":
        diff.time_conditioning = True
        match = "sigma"
    elif what == "sample_ids":
        kw["sample_ids"] = torch.zeros_like(x0)
        match = "sample_ids"
    elif what == "ar":
        diff.parameterization = "ar"
        match = "parameterization=ar"
    elif what == "attention_caching":
        match = "attention_caching"
    else:
        kw["modality"] = 1 - mod
        match = "static slice"
    with pytest.raises(NotImplementedError, match=match):
        diff.sample(**kw)
    assert diff.backbone._cc is None and getattr(diff, "_cond", None) is None


def test_backbone_refusals(doubles):
    g, diff = U.cond_product("cpu")
    bb = diff.backbone
    L = g.case["txt_length"] + g.case["img_length"]
    bb.time_conditioning = True
    with pytest.raises(NotImplementedError, match="sigma"):
        bb.set_conditioning_cache(B, L, "cpu", given="text")
    bb.time_conditioning = False
    bb.causal = True
    with pytest.raises(NotImplementedError, match="bidirectional"):
        bb.set_conditioning_cache(B, L, "cpu", given="text")
    bb.causal = False
    bb.require_sample_ids = True
    with pytest.raises(NotImplementedError, match="unpacked"):
        bb.set_conditioning_cache(B, L, "cpu", given="image")
    bb.require_sample_ids = False
    sl, bb.static_txt_sl = bb.static_txt_sl, slice(L - g.case["txt_length"], None)
    with pytest.raises(NotImplementedError, match="static slice"):
        bb.set_conditioning_cache(B, L, "cpu", given="text")
    bb.static_txt_sl = sl
    with pytest.raises(ValueError, match="given="):
        bb.set_conditioning_cache(B, L, "cpu", given="audio")
    with pytest.raises(ValueError, match="model.length"):
        bb.set_conditioning_cache(B, L - 8, "cpu", given="text")
    assert bb._cc is None
    bb.set_conditioning_cache(B, L, "cpu", given="image", guided=True)
    assert bb._cc.R == 2 * B and bb._cc.sl == slice(0, g.case["txt_length"]) and bb._mc is None      # the modality cache of eval.attention_caching is another one
    with pytest.raises(ValueError, match="conditioning_cache='rebuild'"):
        bb.forward_masked_logits(torch.zeros(2 * B, L, dtype=torch.int64), conditioning_cache="rebuild")
    bb.reset_kv_cache()
    assert bb._cc is None
