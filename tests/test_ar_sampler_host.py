"""CPU checks of the AR sampler's host side (`_ar_sampler`, model_eval.py:2736-2822): its signature, the refusals (each names its key), the BOS rule, the
fixed-prefix length that is prefilled, and the top-p restatement against the reference's `nucleus_sampling` formula.  The kernels and the sampler's
numerics run on the GPU (tests/test_gpu_ar_decode_kernels.py, tests/test_gpu_ar_sampler.py)."""
import inspect
import types

import pytest
import torch

from ar_utils import ar_config
from oracle.cases import CASES
from product_utils import product_config


def _diff(case="b_small", **model_kw):
    from unidisc_amd import Diffusion

    cfg = ar_config(CASES[case])
    for k, v in model_kw.items():
        setattr(cfg.model, k, v)
    return Diffusion(cfg, None, "cpu")


def test_ar_sampler_signature_is_the_reference_one():
    from unidisc_amd import Diffusion

    params = list(inspect.signature(Diffusion._ar_sampler).parameters.values())
    assert [p.name for p in params[:5]] == ["self", "B", "x0", "x0_unmask", "modality"]
    assert all(p.default is None for p in params[2:5])
    assert params[-1].kind is inspect.Parameter.VAR_KEYWORD
    assert {"noise", "seed", "bos_token_id"} <= {p.name for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD}


def test_use_kv_cache_is_accepted_on_causal_and_refused_on_bidirectional():
    from unidisc_amd import Diffusion

    assert _diff(use_kv_cache=True).backbone.use_kv_cache
    cfg = product_config(CASES["b_small"])
    cfg.model.use_kv_cache = True
    with pytest.raises(NotImplementedError, match="use_kv_cache"):
        Diffusion(cfg, None, "cpu")
    cfg = ar_config(CASES["b_small"])
    cfg.model.use_flex_attention_cache = True
    with pytest.raises(NotImplementedError, match="use_flex_attention_cache"):
        Diffusion(cfg, None, "cpu")


def test_reset_kv_cache_refuses_bidirectional_and_keeps_the_probe_form():
    from unidisc_amd import Diffusion

    d = Diffusion(product_config(CASES["b_small"]), None, "cpu")
    d.backbone.reset_kv_cache()    # eval.attention_caching's call: no state
    assert d.backbone._kv is None
    with pytest.raises(NotImplementedError, match="causal"):
        d.backbone.reset_kv_cache(batch_size=2, seq_len=8, dtype=torch.bfloat16, device="cpu")


def test_cached_forward_refusals():
    d = _diff()
    bb = d.backbone
    x = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="reset_kv_cache"):
        bb(x, None, start_pos=0)
    bb._kv = types.SimpleNamespace(B=2, Bp=8, Lmax=31)   # (a cache stand-in: the checks run before any kernel)
    with pytest.raises(NotImplementedError, match="start_pos=4"):
        bb(x, None, start_pos=4)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        bb(x, None, start_pos=0, attention_mask=torch.ones(2, 3, dtype=torch.bool))
    bb._kv = None


def test_sampler_refuses_cpu_first():
    d = _diff()
    with pytest.raises(NotImplementedError, match="AR sampler runs on the GPU only"):
        d._ar_sampler(2)
    d.config.eval.cfg = 1.5   # (even with a configuration it would refuse for another reason)
    with pytest.raises(NotImplementedError, match="AR sampler"):
        d.sample(batch_size=2, x0=torch.zeros(2, 32, dtype=torch.int64), x0_unmask=torch.zeros(2, 32, dtype=torch.bool))


def test_cfg_without_force_cfg_value_is_refused():
    d = _diff()
    d.device = torch.device("cuda")   # past the device check: the configuration check comes before any GPU work
    d.config.eval.cfg = 1.5
    with pytest.raises(NotImplementedError, match="force_cfg_value"):
        d._ar_sampler(2, x0=torch.zeros(2, 32, dtype=torch.int64), x0_unmask=torch.zeros(2, 32, dtype=torch.bool), bos_token_id=1)


def test_bos_resolution():
    d = _diff()
    d.tokenizer = types.SimpleNamespace(bos_token_id=5)
    assert d._ar_bos_id(7) == 5
    d.tokenizer = types.SimpleNamespace(bos_token_id=None)
    assert d._ar_bos_id(7) == 7
    d.tokenizer = None
    assert d._ar_bos_id(0) == 0
    with pytest.raises(ValueError, match="bos_token_id"):
        d._ar_bos_id(None)


def test_fixed_prefix():
    from unidisc_amd import Diffusion

    L = 10
    assert Diffusion._ar_fixed_prefix(None, L) == 1
    u = torch.zeros(3, L, dtype=torch.bool)
    assert Diffusion._ar_fixed_prefix(u, L) == 1
    u[:, :4] = True
    assert Diffusion._ar_fixed_prefix(u, L) == 4
    u[1, 2] = False                  # one row breaks the run at position 2
    assert Diffusion._ar_fixed_prefix(u, L) == 2
    u[:, 0] = False                  # position 0 is fixed either way (BOS)
    assert Diffusion._ar_fixed_prefix(u, L) == 2
    assert Diffusion._ar_fixed_prefix(torch.ones(3, L, dtype=torch.bool), L) == L - 1


def _reference_nucleus(logits, top_p, temperature):
    """model_eval.py:2691-2734 `nucleus_sampling`, restated for the comparison (its last step draws; here the kept, renormalised distribution)"""
    probs = torch.nn.functional.softmax(logits / temperature, dim=-1)
    sp, si = torch.sort(probs, descending=True, dim=-1)
    mask = torch.cumsum(sp, dim=-1) <= top_p
    mask[..., 0] = True
    fp = sp * mask.float()
    fp /= fp.sum(dim=-1, keepdim=True)
    return torch.zeros_like(probs).scatter(-1, si, fp)


def test_top_p_restatement_matches_reference_formula():
    from unidisc_amd import Diffusion

    gen = torch.Generator().manual_seed(0)
    z = torch.randn(4, 50, generator=gen) * 2
    z[:, 7] = float("-inf")      # excluded ids
    # log-softmax (what the reference feeds) and raw logits give the same nucleus: shift invariance
    ref = _reference_nucleus(torch.log_softmax(z, -1), 0.7, 0.8)
    assert (ref[:, 7] == 0).all()
    n = 20000
    for r in range(4):
        ids = Diffusion._ar_nucleus(z[r:r + 1].expand(n, 50), 0.7, 0.8, torch.Generator().manual_seed(r))
        assert (ref[r, ids] > 0).all()       # every draw lies in the nucleus
        freq = torch.bincount(ids, minlength=50).float() / n
        assert float((freq - ref[r]).abs().max()) < 0.02


def test_sample_refuses_what_the_ar_sampler_does_not_take():
    d = _diff()
    d.device = torch.device("cuda")   # past the device check: the argument checks come before any GPU work
    L = d.config.model.length
    for kw, key in ((dict(sample_ids=torch.zeros(2, L, dtype=torch.int64)), "sample_ids"), (dict(replay=[None]), "replay"),
                    (dict(predictor="maskgit"), "predictor"), (dict(num_steps=5), "num_steps")):
        with pytest.raises(NotImplementedError, match=key):
            d.sample(batch_size=2, **kw)


def test_decode_cache_refuses_time_conditioning():
    from unidisc_amd.dit import DIT

    d = _diff()
    bb = d.backbone
    bb.time_conditioning = True     # (a causal DIT built with adaLN directly: the Diffusion level refuses it for AR)
    with pytest.raises(NotImplementedError, match="time_conditioning"):
        DIT.reset_kv_cache(bb, batch_size=2, seq_len=8, dtype=torch.bfloat16, device="cpu")
