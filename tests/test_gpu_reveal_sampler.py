"""eval.fused_reveal and trainer.force_after_eos_padding on a real MI355X (pytest -m gpu): `Diffusion.sample()` with replayed draws gives the same tokens bit for
bit with the fused step tail (`udm_reveal_rows`) as with the tensor statements - maskgit, maskgit_nucleus, first_hitting, guided and unguided, with and without
the padding behind EOS, and ddpm_cache with the padding (the pad-only call); the recorded reference run is still reached; the fused tail makes no synchronising
call.  The kernel itself is held to tests/reveal_ref.py in tests/test_gpu_reveal_rows.py."""
import os

import numpy as np
import pytest
import torch

from golden_utils import GOLDEN_DIR, Golden
from product_utils import build_product
from test_sampler import AGREE_BOUNDS

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Tok:
    def __init__(self, eos, pad, bos):
        self.eos_token_id, self.pad_token_id, self.bos_token_id = eos, pad, bos


def _load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if z[k].dtype.kind != "U"}


def _fixture(predictor, case):
    s = _load(f"{predictor}_{case}")
    steps = int(s["steps"])
    if predictor == "first_hitting":
        replay = [(s[f"step{i}/u"].to(DEV), s[f"step{i}/pos_u"].to(DEV) if f"step{i}/pos_u" in s else None) for i in range(steps)]
    else:
        replay = [(s[f"step{i}/pred"].to(DEV), s[f"step{i}/gumbel"].float().to(DEV)) if f"step{i}/pred" in s else (None, None) for i in range(steps)]
    kw = dict(num_steps=steps, eps=float(s["eps"]), batch_size=s["x_init"].shape[0], modality=s["modality"].to(DEV) if "modality" in s else None,
              x0=s["x0"].to(DEV) if "x0" in s else None, x0_unmask=s["x0_unmask"].bool().to(DEV) if "x0" in s else None, predictor=predictor, replay=replay)
    return s, kw


def _eos_for(s, Lt):
    """an EOS id the replayed run is sure to draw: the recorded final token of sample 0 at its first free text position (l); a pad id that differs"""
    free = ~s["x0_unmask"].bool()[0, :Lt] if "x0_unmask" in s else torch.ones(Lt, dtype=torch.bool)
    if not bool(free.any()):      # the whole text is given (the c_large runs): an EOS inside the given text, whose tail the write-back restores
        eos = int(s["x0"][0, Lt // 2])
        return None, eos, (0 if eos != 0 else 1)
    l = int(free.nonzero()[0])
    eos = int(s["x_before_noise_removal"][0, l])
    return l, eos, (0 if eos != 0 else 1)


def _run(g, s, kw, *, fused, padding, cfg=None, eos=None, pad=None):
    from unidisc_amd.config import Cfg

    diff = build_product(g, device=DEV)
    diff.backbone.eval()
    ev = dict(fused_reveal=fused)
    for k in ("r_temp", "top_p", "temperature"):
        if k in s:
            ev["maskgit_r_temp" if k == "r_temp" else k] = float(s[k])
    if cfg is not None:
        ev.update(cfg=cfg)
    diff.config.eval = Cfg(**ev)
    if padding:
        diff.config.trainer.force_after_eos_padding = True
        diff.tokenizer = Tok(eos, pad, None)
    return diff, diff.sample(return_nfe=True, seed=3, **kw)


CASES = [("maskgit", "c_large"), ("maskgit", "b_small"), ("maskgit_nucleus", "c_large"), ("first_hitting", "c_large"), ("first_hitting", "b_small")]


# guidance needs conditioning: the c_large runs have x0, the b_small runs are unconditional
RUNS = [(p, c, guided, padding) for p, c in CASES for guided in ((False, True) if c == "c_large" else (False,)) for padding in (False, True)]


@pytest.mark.parametrize("predictor,case,guided,padding", RUNS, ids=[f"{p}-{c}-{'guided' if gd else 'unguided'}-{'pad' if pd else 'nopad'}" for p, c, gd, pd in RUNS])
def test_fused_reveal_equals_the_tensor_path(predictor, case, guided, padding):
    g = Golden(case)
    s, kw = _fixture(predictor, case)
    assert (kw["x0"] is not None) == (case == "c_large")
    Lt = g.case["txt_length"]
    l, eos, pad = _eos_for(s, Lt)
    if padding and predictor != "first_hitting" and l is not None:      # plant the EOS: whichever step reveals position (0, l) reveals it there
        kw["replay"] = [(None, None) if p is None else (torch.cat([p[:1].clone().index_fill_(1, torch.tensor([l], device=DEV), eos), p[1:]], 0), gm) for p, gm in kw["replay"]]
    seen = []
    outs = []
    for fused in (False, True):
        from unidisc_amd import diffusion as diff_mod

        real = diff_mod.K.reveal_rows
        diff_mod.K.reveal_rows = lambda *a, _real=real, **k: (seen.append(k.get("eos_id")), _real(*a, **k))[1]
        try:
            diff, out = _run(g, s, kw, fused=fused, padding=padding, cfg=2.0 if guided else None, eos=eos, pad=pad)
        finally:
            diff_mod.K.reveal_rows = real
        assert bool(seen) == fused and all(e == (eos if padding else None) for e in seen)
        outs.append(out)
    (x_off, nfe_off), (x_on, nfe_on) = outs
    assert torch.equal(x_on, x_off) and nfe_on == nfe_off
    assert not bool((x_on == diff.mask_index).any())
    if kw["x0"] is not None:
        assert torch.equal(x_on[kw["x0_unmask"]], kw["x0"][kw["x0_unmask"]])
    if padding and predictor != "first_hitting" and l is not None:      # the token at (0, l) is the EOS: the free text behind it is pad
        free = ~kw["x0_unmask"][0, :Lt] if kw["x0"] is not None else torch.ones(Lt, dtype=torch.bool, device=DEV)
        behind = x_on[0, l + 1:Lt][free[l + 1:]]
        assert bool((behind == pad).all()) and behind.numel() > 0
    if not padding and not guided:                    # the recorded reference run is still reached with the key on
        key = {"maskgit": "test_maskgit_loop_on_gpu", "maskgit_nucleus": "test_maskgit_nucleus_loop_on_gpu", "first_hitting": "test_first_hitting_loop_on_gpu"}[predictor]
        key = key if predictor == "maskgit_nucleus" else f"{key}[{case}]"
        dis = 1.0 - (x_on.cpu() == s["x_final"]).float().mean().item()
        print(f"{predictor} {case}: token disagreement with the recorded run {dis:.4f}")
        assert dis <= AGREE_BOUNDS.get(key, 0.02) and nfe_on == int(s["nfe"]) + 1


@pytest.mark.parametrize("case", ["c_large", "b_small"])
def test_ddpm_cache_pads_through_the_kernel(case):
    """ddpm_cache with trainer.force_after_eos_padding: the pad-only call against the tensor statements, free-running on the same seed"""
    g = Golden(case)
    s, kw = _fixture("maskgit", case)
    kw = dict(kw, predictor="ddpm_cache", replay=None, num_steps=8)
    eos, pad = 5, 0
    (d0, (x_off, nfe_off)), (d1, (x_on, nfe_on)) = (_run(g, s, kw, fused=f, padding=True, eos=eos, pad=pad) for f in (False, True))
    assert torch.equal(x_on, x_off) and nfe_on == nfe_off
    _, (x_free, _) = _run(g, s, kw, fused=True, padding=False)
    Lt = g.case["txt_length"]
    has = (x_free[:, : Lt - 1] == eos).any()
    print(f"{case}: EOS drawn without the padding key: {bool(has)}; pads with it: {int((x_on[:, :Lt] == pad).sum())}")


@pytest.mark.parametrize("lottery", [False, True], ids=["confidence", "lottery"])
def test_fused_tail_makes_no_synchronising_call(lottery):
    """the probe of tests/test_gpu_nucleus_sampler.py on the step tail: `_maskgit_reveal` / the first_hitting call with the fused operands under torch's sync
    debug mode - no `int(num_unmask.max())`, no other host read"""
    from unidisc_amd.config import Cfg

    g = Golden("c_large")
    diff = build_product(g, device=DEV)
    diff.config.eval = Cfg(fused_reveal=True, maskgit_r_temp=10.0)
    B, L, Lt = 4, g.case["txt_length"] + g.case["img_length"], g.case["txt_length"]
    gen = torch.Generator().manual_seed(2)
    x = torch.randint(3, 30, (B, L), generator=gen)
    x[torch.rand(B, L, generator=gen) < 0.5] = diff.mask_index
    rows = (x.reshape(-1) == diff.mask_index).nonzero().reshape(-1)
    n = rows.numel()
    mod = torch.zeros(B, L, dtype=torch.int64)
    mod[:, Lt:] = 1
    x0_unmask = x != diff.mask_index
    dev = lambda t: t.to(DEV)
    x, rows, mod, x0_unmask = dev(x), dev(rows), dev(mod), dev(x0_unmask)
    tok, logp = dev(torch.randint(3, 30, (n,), generator=gen)), dev(-torch.rand(n, generator=gen))
    k = torch.full((B,), 3, dtype=torch.int64, device=DEV)
    t_col = torch.full((B, 1), 0.5, device=DEV)
    noise = dev(torch.rand(B, L, generator=gen))
    tail = dict(eos_id=5, pad_id=0, modality=mod, x0=x.clone(), x0_unmask=x0_unmask)

    def step(nz):
        if lottery:
            from unidisc_amd import kernels as K
            return K.reveal_rows(x, diff.mask_index, rows=rows, tok=tok, sched=k, noise=nz, seed=4, lottery=True, **tail)
        return diff._maskgit_reveal(x, x != diff.mask_index, k, rows, tok, logp, nz, 3, 10.0, t_col, tail=tail)[0]

    step(noise)   # (warm-up: first launch, allocator)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = step(noise), step(None)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert int(((a != x) & (x == diff.mask_index)).sum()) >= B and int(((b != x) & (x == diff.mask_index)).sum()) >= B
