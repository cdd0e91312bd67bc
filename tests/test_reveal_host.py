"""CPU checks of the host side of `trainer.force_after_eos_padding` and `eval.fused_reveal` with kernel doubles (tests/fake_kernels_reveal.py): the padding
behind the first EOS through `Diffusion.sample()` for all four predictors against tests/reveal_ref.py, step by step; the fused tail handed the same operands and
giving the same tokens; the reference's no-op conditions; the ValueError; and that nothing changes with both keys unset."""
import pytest
import torch

import fake_kernels_reveal as FK
import reveal_ref as R
from golden_utils import Golden
from product_utils import build_product

PREDICTORS = ("ddpm_cache", "maskgit", "maskgit_nucleus", "first_hitting")
EOS, PAD, BOS = 2, 0, 1
STEPS = 4


class Tok:
    def __init__(self, eos=EOS, pad=PAD, bos=BOS):
        self.eos_token_id, self.pad_token_id, self.bos_token_id = eos, pad, bos


def _product(monkeypatch, *, padding=True, fused=False, tokenizer=Tok(), **ev):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod
    from unidisc_amd.config import Cfg

    monkeypatch.setattr(dit_mod, "K", FK)
    monkeypatch.setattr(diff_mod, "K", FK)
    g = Golden("c_large")
    diff = build_product(g, device="cpu")
    diff.backbone.eval()
    diff.tokenizer = tokenizer
    diff.config.eval = Cfg(maskgit_r_temp=10.0, top_p=0.95, temperature=0.9, **ev)
    if fused is not None:
        diff.config.eval.fused_reveal = fused
    if padding is not None:
        diff.config.trainer.force_after_eos_padding = padding
    FK.REVEAL_CALLS.clear()
    return diff, g


def _inputs(diff, g, family, B=2):
    """(x0, x0_unmask, modality, replay per predictor): the draws are replayed, so an EOS can be planted where the family wants it"""
    L, Lt = g.case["txt_length"] + g.case["img_length"], g.case["txt_length"]
    gen = torch.Generator().manual_seed(11 + len(family))
    modality = torch.zeros(B, L, dtype=torch.int64)
    modality[:, Lt:] = 1
    Vt, V = g.case["text_vocab_size"], g.case["vocab_size"]
    pred = torch.cat([torch.randint(3, Vt - 1, (B, Lt), generator=gen), torch.randint(Vt, V, (B, L - Lt), generator=gen)], 1)
    x0 = x0_unmask = None
    if family == "eos_at_0":
        pred[:, 0] = EOS
    elif family == "eos_last_text":
        pred[:, Lt - 1] = EOS
    elif family in ("eos_revealed", "drawn"):
        pred[:, 2] = EOS
    elif family == "eos_several":
        pred[:, 1:Lt:3] = EOS
    elif family == "eos_in_x0":      # given text: an EOS in the middle, given tokens behind it, free text positions at the end
        x0 = pred.clone()
        x0[:, Lt // 2] = EOS
        x0_unmask = torch.zeros(B, L, dtype=torch.bool)
        x0_unmask[:, : Lt - 3] = True
    else:
        assert family == "eos_absent"
    gumbel = [torch.randn(B, L, generator=gen) for _ in range(STEPS)]
    pos_u = [torch.rand(B, L, generator=gen) for _ in range(STEPS)]
    if family in ("eos_revealed", "drawn"):
        for s in gumbel:
            s[:, 2] = 50.0           # the planted EOS wins the first step
        for s in pos_u:
            s[:, 2] = 2.0
    return dict(x0=x0, x0_unmask=x0_unmask, modality=modality, batch_size=B), dict(maskgit=[(pred, s) for s in gumbel], maskgit_nucleus=[(pred, s) for s in gumbel],
                                                                                   first_hitting=[(None, s) for s in pos_u], ddpm_cache=None), pred


def _record_updates(monkeypatch, diff):
    """(x before the update, x the update returned) of every step"""
    seen = []
    for name in ("_maskgit_update", "_first_hitting_update", "_ddpm_caching_update"):     # (the nucleus update is `_maskgit_update` with a draw rule)
        real = getattr(diff, name)

        def wrapped(x, *a, _real=real, _name=name, **kw):
            out = _real(x, *a, **kw)
            seen.append((x.clone(), (out[1] if _name == "_ddpm_caching_update" else out[0]).clone()))
            return out

        monkeypatch.setattr(diff, name, wrapped)
    return seen


FAMILIES = ("eos_absent", "eos_at_0", "eos_last_text", "eos_revealed", "eos_several", "eos_in_x0")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("predictor", PREDICTORS)
def test_padding_follows_the_rule_step_by_step(monkeypatch, predictor, family):
    """tensor path: after every update the state is reveal_ref's pad-only form (padding, then write-back) of what the update returned"""
    diff, g = _product(monkeypatch)
    kw, replay, pred = _inputs(diff, g, family)
    seen = _record_updates(monkeypatch, diff)
    x = diff.sample(num_steps=STEPS, predictor=predictor, replay=replay[predictor], seed=3, noise_removal=False, **kw)
    assert len(seen) == STEPS and not FK.REVEAL_CALLS
    rule = lambda v: R.reveal_ref(v, diff.mask_index, eos_id=EOS, pad_id=PAD, modality=kw["modality"], x0=kw["x0"], x0_unmask=kw["x0_unmask"])
    for i, (_, out) in enumerate(seen):
        nxt = seen[i + 1][0] if i + 1 < STEPS else x
        assert torch.equal(nxt, rule(out)), f"step {i}"
    if kw["x0"] is not None:
        assert torch.equal(x[kw["x0_unmask"]], kw["x0"][kw["x0_unmask"]])     # the write-back restores given tokens behind the given EOS
    hit = any(not torch.equal(rule(out), out if kw["x0"] is None else torch.where(kw["x0_unmask"], kw["x0"], out)) for _, out in seen)
    if predictor != "ddpm_cache" and family not in ("eos_absent", "eos_last_text"):
        assert hit, "the family never made the rule pad anything"


def test_tokens_behind_a_drawn_eos_are_pad(monkeypatch):
    """trainer.force_after_eos_padding set: the text behind an EOS the sampler drew is pad, the EOS itself, the text before it and the image are not"""
    diff, g = _product(monkeypatch)
    kw, replay, pred = _inputs(diff, g, "drawn")
    Lt = g.case["txt_length"]
    x = diff.sample(num_steps=STEPS, predictor="maskgit", replay=replay["maskgit"], seed=3, noise_removal=False, **kw)
    assert bool((x[:, 2] == EOS).all())
    behind = x[:, 3:Lt]
    assert bool(((behind == PAD) | (behind == diff.mask_index)).all()) and bool((behind == PAD).any()), behind
    assert not bool((x[:, Lt:] == PAD).any()) and not bool((x[:, :2] == PAD).any())
    y = diff.sample(num_steps=STEPS, predictor="maskgit", replay=replay["maskgit"], seed=3, **kw)     # the noise removal pads nothing (as in the reference)
    assert bool((y[:, 2] == EOS).all()) and not bool((y == diff.mask_index).any())
    still = x[:, 3:Lt] == diff.mask_index
    assert bool((y[:, 3:Lt][~still] == PAD).all())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("predictor", PREDICTORS)
@pytest.mark.parametrize("padding", [True, False], ids=["pad", "nopad"])
def test_fused_tail_equals_the_tensor_path(monkeypatch, predictor, family, padding):
    outs = []
    for fused in (False, True):
        diff, g = _product(monkeypatch, padding=padding, fused=fused)
        kw, replay, _ = _inputs(diff, g, family)
        outs.append(diff.sample(num_steps=STEPS, predictor=predictor, replay=replay[predictor], seed=3, return_nfe=True, **kw))
        calls = list(FK.REVEAL_CALLS)
        if not fused:
            assert not calls
            continue
        if predictor == "ddpm_cache":     # the pad-only call, and only with the padding key
            assert len(calls) == (STEPS if padding else 0) and all(c["n"] == 0 and c["sched"] is None for c in calls)
        else:
            assert len(calls) == STEPS and any(c["n"] > 0 for c in calls)
            assert all(c["lottery"] == (predictor == "first_hitting") and c["noise"] for c in calls if c["n"] > 0)
        assert all((c["eos_id"], c["pad_id"]) == ((EOS, PAD) if padding else (None, None)) and c["x0"] == (kw["x0"] is not None) for c in calls)
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_fused_tail_makes_no_host_read(monkeypatch):
    """`int(num_unmask.max())` is gone from the fused tail: the tensor statements of today's tail never run"""
    diff, g = _product(monkeypatch, fused=True)
    kw, replay, _ = _inputs(diff, g, "eos_several")
    monkeypatch.setattr(torch, "topk", lambda *a, **k: pytest.fail("torch.topk ran with eval.fused_reveal on"))
    monkeypatch.setattr(type(diff), "_first_hitting_reveal", staticmethod(lambda *a, **k: pytest.fail("the tensor lottery ran with eval.fused_reveal on")))
    monkeypatch.setattr(type(diff), "_pad_after_eos", lambda *a, **k: pytest.fail("the tensor padding ran with eval.fused_reveal on"))
    for predictor in PREDICTORS:
        diff.sample(num_steps=STEPS, predictor=predictor, replay=replay[predictor], seed=3, **kw)


def test_free_running_fused_sampler_completes_and_is_seeded(monkeypatch):
    diff, g = _product(monkeypatch, fused=True)
    kw, _, _ = _inputs(diff, g, "eos_absent")
    for predictor in ("maskgit", "first_hitting"):
        a = diff.sample(num_steps=STEPS, predictor=predictor, seed=3, **kw)
        b = diff.sample(num_steps=STEPS, predictor=predictor, seed=3, **kw)
        c = diff.sample(num_steps=STEPS, predictor=predictor, seed=4, **kw)
        assert torch.equal(a, b) and not torch.equal(a, c) and not (a == diff.mask_index).any()


@pytest.mark.parametrize("fused", [False, True])
def test_no_op_conditions(monkeypatch, fused):
    """model_eval.py:2390: no padding when the tokenizer's EOS is its BOS, and none under eval.attention_caching"""
    diff, g = _product(monkeypatch, fused=fused, tokenizer=Tok(bos=EOS))
    kw, replay, _ = _inputs(diff, g, "drawn")
    monkeypatch.setattr(type(diff), "_pad_after_eos", lambda *a, **k: pytest.fail("padding ran although eos == bos"))
    x = diff.sample(num_steps=STEPS, predictor="maskgit", replay=replay["maskgit"], seed=3, **kw)
    assert not bool((x[:, : g.case["txt_length"]] == PAD).any()) and all(c["eos_id"] is None for c in FK.REVEAL_CALLS)
    diff2, _ = _product(monkeypatch, fused=fused, attention_caching=True, attention_caching_txt_to_img_ratio=2)
    monkeypatch.setattr(type(diff2), "_pad_after_eos", lambda *a, **k: pytest.fail("padding ran under eval.attention_caching"))
    assert diff2._eos_padding_ids(True) is None
    diff2.sample(num_steps=STEPS, predictor="ddpm_cache", batch_size=2, modality=kw["modality"], seed=3)
    assert not FK.REVEAL_CALLS


def test_ids_come_from_the_tokenizer_then_from_the_config_keys(monkeypatch):
    diff, _ = _product(monkeypatch)
    assert diff._eos_padding_ids(False) == (EOS, PAD)
    diff, _ = _product(monkeypatch, tokenizer=None, eos_token_id=7, pad_token_id=9)
    assert diff._eos_padding_ids(False) == (7, 9)
    diff, _ = _product(monkeypatch, tokenizer=Tok(eos=None), eos_token_id=7)
    assert diff._eos_padding_ids(False) == (7, PAD)
    diff, _ = _product(monkeypatch, padding=False, tokenizer=None)
    assert diff._eos_padding_ids(False) is None
    diff, _ = _product(monkeypatch, padding=None, tokenizer=None)
    assert diff._eos_padding_ids(False) is None


@pytest.mark.parametrize("tokenizer,ev,names", [(None, {}, ("eval.eos_token_id", "eval.pad_token_id", "neither")), (Tok(eos=None), {}, ("eval.eos_token_id", "EOS id")),
                                                (None, dict(eos_token_id=3), ("eval.pad_token_id", "pad id"))])
def test_missing_ids_raise(monkeypatch, tokenizer, ev, names):
    diff, g = _product(monkeypatch, tokenizer=tokenizer, **ev)
    with pytest.raises(ValueError) as e:
        diff.sample(num_steps=2, predictor="maskgit", batch_size=2, seed=3)
    assert "force_after_eos_padding" in str(e.value) and all(n in str(e.value) for n in names)


@pytest.mark.parametrize("predictor", PREDICTORS)
def test_keys_unset_nothing_changes(monkeypatch, predictor):
    """both keys unset (or false): no padding statement, no fused call, and the tokens of a run with the keys absent"""
    outs = []
    for padding, fused in ((None, None), (False, False)):
        diff, g = _product(monkeypatch, padding=padding, fused=fused, tokenizer=None)
        kw, replay, _ = _inputs(diff, g, "eos_several")
        monkeypatch.setattr(type(diff), "_pad_after_eos", lambda *a, **k: pytest.fail("padding ran with the key unset"))
        monkeypatch.setattr(FK, "reveal_rows", lambda *a, **k: pytest.fail("udm_reveal_rows ran with the key unset"))
        outs.append(diff.sample(num_steps=STEPS, predictor=predictor, replay=replay[predictor], seed=3, **kw))
    assert torch.equal(outs[0], outs[1])
    if predictor.startswith("maskgit"):      # (replayed tokens: the planted EOS is there and the text behind it is not padded)
        assert bool((outs[0][:, 1] == EOS).all()) and not bool((outs[0][:, 2: g.case["txt_length"]] == PAD).any())


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("predictor", PREDICTORS)
def test_conditioning_cache_pads_the_sliced_state(monkeypatch, predictor, fused):
    """eval.conditioning_cache with the image given: from step 1 on the state is the text slice, and the rule runs on it with the sliced modality - the tokens
    are those of the run without the cache key's slicing of the rule, i.e. reveal_ref's padding of every step on whatever the state then is"""
    import conditioning_cache_utils as U

    diff, g = _product(monkeypatch, fused=fused, conditioning_cache=True)
    x0, unmask, mod, sl = U.conditioning(g, diff, 2, "image")
    Lt = g.case["txt_length"]
    assert (sl.start, sl.stop) == (0, Lt)
    seen = _record_updates(monkeypatch, diff)
    x = diff.sample(num_steps=STEPS, x0=x0, x0_unmask=unmask, modality=mod, predictor=predictor, seed=5, noise_removal=False)
    assert diff.sample_step_modes == ["build"] + ["slice"] * (STEPS - 1) and [tuple(a.shape)[1] for a, _ in seen] == [x0.shape[1]] + [Lt] * (STEPS - 1)
    for i, (_, out) in enumerate(seen):
        cut = (lambda v: v) if out.shape[1] == x0.shape[1] else (lambda v: v[:, sl])
        want = R.reveal_ref(out, diff.mask_index, eos_id=EOS, pad_id=PAD, modality=cut(mod), x0=cut(x0), x0_unmask=cut(unmask))
        nxt = seen[i + 1][0] if i + 1 < STEPS else x[:, sl]
        assert torch.equal(nxt[:, -want.shape[1]:] if nxt.shape[1] < want.shape[1] else nxt, want if nxt.shape[1] == want.shape[1] else want[:, sl]), f"step {i}"
    assert torch.equal(x[unmask], x0[unmask])
    if fused:
        assert [c["shape"][1] for c in FK.REVEAL_CALLS] == [x0.shape[1]] + [Lt] * (STEPS - 1) and all(c["eos_id"] == EOS for c in FK.REVEAL_CALLS)
