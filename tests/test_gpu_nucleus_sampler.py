"""eval.fused_nucleus on a real MI355X (pytest -m gpu): the maskgit_nucleus loop and the AR sampler's top-p branch on the fused kernels
(udm_nucleus_sample_rows, udm_ar_nucleus_rows).  The kernels themselves are held to fp64 in tests/test_gpu_nucleus_rows.py; here the samplers around them."""
import os

import numpy as np
import pytest
import torch

from ar_utils import ar_config
from golden_utils import GOLDEN_DIR, Golden
from oracle import unidisc_oracle as O
from oracle.cases import CASES
from product_utils import build_product

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _golden():
    z = np.load(os.path.join(GOLDEN_DIR, "maskgit_nucleus_c_large.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if z[k].dtype.kind != "U"}


def _count(monkeypatch, names):
    """counts of K.<name> calls made by the samplers"""
    from unidisc_amd import diffusion as diff_mod

    seen = {n: 0 for n in names}
    for n in names:
        real = getattr(diff_mod.K, n)

        def wrapped(*a, _real=real, _n=n, **kw):
            seen[_n] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(diff_mod.K, n, wrapped)
    return seen


def test_maskgit_nucleus_loop_fused(monkeypatch):
    from unidisc_amd.config import Cfg

    g, s = Golden("c_large"), _golden()
    diff = build_product(g, device=DEV)
    diff.backbone.eval()
    steps = int(s["steps"])
    diff.config.eval = Cfg(maskgit_r_temp=float(s["r_temp"]), top_p=float(s["top_p"]), temperature=float(s["temperature"]), fused_nucleus=True)
    monkeypatch.setattr(type(diff), "_nucleus_draw", lambda self, *a, **kw: pytest.fail("_nucleus_draw ran with eval.fused_nucleus on"))
    seen = _count(monkeypatch, ["nucleus_sample_rows", "categorical_sample_rows"])
    B = 4
    x0, x0_unmask, mod = s["x0"].to(DEV).expand(B, -1), s["x0_unmask"].bool().to(DEV).expand(B, -1), s["modality"].to(DEV).expand(B, -1).contiguous()
    a, nfe = diff.sample(num_steps=steps, x0=x0, x0_unmask=x0_unmask, batch_size=B, modality=mod, predictor="maskgit_nucleus", seed=3, return_nfe=True)
    assert seen["nucleus_sample_rows"] == nfe - 1 >= 2 and seen["categorical_sample_rows"] == 0       # one fused call per step, no given= pass
    assert not (a == diff.mask_index).any() and torch.equal(a[x0_unmask], x0[x0_unmask])
    b = diff.sample(num_steps=steps, x0=x0, x0_unmask=x0_unmask, batch_size=B, modality=mod, predictor="maskgit_nucleus", seed=3)
    c = diff.sample(num_steps=steps, x0=x0, x0_unmask=x0_unmask, batch_size=B, modality=mod, predictor="maskgit_nucleus", seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # unconditional, as tests/test_sampler.py::test_maskgit_nucleus_loop_on_gpu runs it
    u1 = diff.sample(num_steps=steps, batch_size=B, modality=mod, predictor="maskgit_nucleus", seed=3)
    u2 = diff.sample(num_steps=steps, batch_size=B, modality=mod, predictor="maskgit_nucleus", seed=3)
    assert torch.equal(u1, u2) and not (u1 == diff.mask_index).any()


def test_fused_step_draws_from_the_oracle_nucleus(monkeypatch):
    """tests/test_sampler.py:367-374 on the fused path: every token of a free step lies in `oracle.nucleus_filter`'s kept set of the step's own distribution"""
    from unidisc_amd import diffusion as diff_mod
    from unidisc_amd.config import Cfg

    g, s = Golden("c_large"), _golden()
    diff = build_product(g, device=DEV)
    diff.backbone.eval()
    top_p, temp = float(s["top_p"]), float(s["temperature"])
    diff.config.eval = Cfg(maskgit_r_temp=float(s["r_temp"]), top_p=top_p, temperature=temp, fused_nucleus=True)
    got = {}
    real = diff_mod.K.nucleus_sample_rows

    def grab(logits, *a, **kw):
        out = real(logits, *a, **kw)
        got.update(logits=logits.clone(), tok=out[0].clone(), logp=out[1].clone(), kw=kw)
        return out

    monkeypatch.setattr(diff_mod.K, "nucleus_sample_rows", grab)
    B = 4
    xs, mod = s["step1/x"].to(DEV).expand(B, -1).contiguous(), s["modality"].to(DEV).expand(B, -1).contiguous()
    t = (s["timesteps"][1] * torch.ones(B, 1)).to(DEV)
    sched = diff.adap_sche(xs, int(s["steps"]), diff.mask_index, "arccos")
    out, _ = diff._maskgit_nucleus_update(xs, t, None, schedule=sched, step=1, modality=mod, seed=5)
    n = got["logits"].shape[0]
    assert n == int((xs == diff.mask_index).sum()) and got["kw"]["inv_temperature"] == 1.0
    rm = got["kw"]["modality"].cpu()
    lp = O.subs_parameterization(g.cfg, got["logits"][:, : g.cfg.vocab_size].float().cpu()[None], torch.full((1, n), g.cfg.mask_index), rm[None], None).float()[0]
    fp = O.nucleus_filter(lp.exp(), top_p, temp)
    tok = got["tok"].cpu()
    assert bool((fp.gather(-1, tok[:, None]) > 0).all())
    assert torch.allclose(got["logp"].cpu(), lp.gather(-1, tok[:, None])[:, 0], atol=2e-5, rtol=1e-5)      # the confidence: log p under the unfiltered distribution
    keep = xs != diff.mask_index
    assert torch.equal(out[keep], xs[keep])


def _ar_diff(seed, **ev):
    from unidisc_amd import Diffusion

    torch.manual_seed(seed)
    diff = Diffusion(ar_config(dict(CASES["b_small"])), None, DEV)
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "embed" in n or "attn" in n or "mlp" in n:
                p.copy_((torch.randn(p.shape, generator=gen) * 2 / p.shape[-1] ** 0.5).to(DEV))
    diff.backbone.eval()
    for k, v in ev.items():
        setattr(diff.config.eval, k, v)
    return diff


def _static_mod(diff, B):
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    mod[:, diff.static_img_sl] = 1
    return mod


def _excluded(diff, nxt_mod):
    V, Vt = diff.vocab_size, diff.text_vocab_size
    ids = torch.arange(V, device=DEV)
    bad = (ids == diff.mask_index)[None, None].expand(*nxt_mod.shape, V)
    if diff._restrict():
        bad = bad | torch.where((nxt_mod == 1)[..., None], ids < Vt, ids >= Vt)
    return bad


def _in_nucleus(z, x, top_p, temp):
    """tests/test_gpu_ar_sampler.py:172-179: the drawn id's nucleus test on the full forward's logits, with that file's tolerance"""
    probs = torch.softmax(z / temp, -1)
    p_tok = probs.gather(-1, x[:, 1:, None])[..., 0]
    mass_above = (probs * (probs > p_tok[..., None])).sum(-1)
    top = probs.max(-1).values
    return (mass_above + p_tok <= top_p + 5e-2) | (p_tok >= top - 1e-4)


@pytest.mark.parametrize("cond", [False, True], ids=["free", "cfg_x0"])
def test_ar_top_p_fused(cond, monkeypatch):
    """Free: the drawn ids against the nucleus of the full causal forward's logits, as tests/test_gpu_ar_sampler.py does for the tensor path.  With guidance
    and x0: against the nucleus of the guided mix of the sampler's own next-token logits (recorded at every step) - the mix (1 + w) l_c - w l_u multiplies
    the bf16 difference between the decode path and the full forward by 1 + 2 w = 4, which the tolerance of that file was not set for (the full-forward
    figure is printed) - under the same tolerance."""
    from unidisc_amd import diffusion as diff_mod

    diff = _ar_diff(3, top_p=0.8, temperature=0.7, fused_nucleus=True)
    monkeypatch.setattr(type(diff), "_ar_nucleus", staticmethod(lambda *a, **kw: pytest.fail("_ar_nucleus ran with eval.fused_nucleus on")))
    B, L, V = 8, diff.config.model.length, diff.vocab_size
    steps = {}
    real = diff_mod.K.ar_nucleus_rows

    def record(logits, x, pos, *a, **kw):
        assert kw["rows"] == B and kw["inv_temperature"] == 1.0 / 0.7 and kw["budget"] == 0.8 and (kw["logits_u"] is not None) == cond
        steps[pos] = logits[: 2 * B if cond else B, :V].float().clone()
        return real(logits, x, pos, *a, **kw)

    monkeypatch.setattr(diff_mod.K, "ar_nucleus_rows", record)
    seen = _count(monkeypatch, ["ar_sample_rows"])
    mod = _static_mod(diff, B)
    x0 = x0_unmask = None
    if cond:
        diff.config.eval.cfg = 1.5
        diff.config.eval.force_cfg_value = True
        gen = torch.Generator().manual_seed(12)
        x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to(DEV)
        x0_unmask = torch.zeros(B, L, dtype=torch.bool, device=DEV)
        x0_unmask[:, :diff.config.model.txt_length // 2] = True
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=5, bos_token_id=3)
    assert nfe == 0 and len(steps) >= 1 and seen["ar_sample_rows"] == 0
    assert not (x == diff.mask_index).any()
    with torch.no_grad():
        z = diff.backbone(x, None, modality=mod).float()
        if cond:
            assert torch.equal(x[x0_unmask], x0[x0_unmask])
            zu = diff.backbone(torch.where(x0_unmask, diff.mask_index, x), None, modality=mod).float()
            z = 2.5 * z - 1.5 * zu
    z = z[:, :-1].masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
    ok = _in_nucleus(z, x, 0.8, 0.7)
    if cond:
        ok = ok | x0_unmask[:, 1:]
    print(f"full-forward nucleus test: {int((~ok).sum())} of {ok.numel()} drawn ids outside")
    if not cond:
        assert ok.all(), int((~ok).sum())
    else:
        assert sorted(steps) == list(range(min(steps), L))          # one launch per decoded position
        zs = torch.full((B, L - 1, V), 0.0, device=DEV)
        own = torch.zeros(B, L - 1, dtype=torch.bool, device=DEV)
        for pos, lg in steps.items():
            zs[:, pos - 1] = (1 + 1.5) * lg[:B] - 1.5 * lg[B:]
            own[:, pos - 1] = True
        zs = zs.masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
        ok2 = _in_nucleus(zs, x, 0.8, 0.7) | x0_unmask[:, 1:] | ~own
        assert ok2.all(), int((~ok2).sum())
    x2, _ = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=5, bos_token_id=3)
    x3, _ = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=6, bos_token_id=3)
    assert torch.equal(x, x2) and not torch.equal(x, x3)


def test_ar_top_p_fused_has_no_host_sync():
    """the probe of tests/test_gpu_ar_sampler.py::test_sampler_has_no_host_sync_and_frees_cache on the fused top-p token loop"""
    diff = _ar_diff(4, top_p=0.8, temperature=0.7, fused_nucleus=True)
    B, L = 4, diff.config.model.length
    mod = _static_mod(diff, B)
    diff._ar_sampler(B, modality=mod, seed=9, bos_token_id=3)   # (warm-up: first launches, allocator)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, nfe = diff._ar_sampler(B, modality=mod, seed=9, bos_token_id=3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert nfe == 0 and not (x[:, 1:] == diff.mask_index).any() and diff.backbone._kv is None
