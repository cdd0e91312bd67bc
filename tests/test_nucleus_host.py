"""CPU checks of the host side of eval.fused_nucleus with kernel doubles (tests/fake_kernels_nucleus.py): off, a maskgit_nucleus step issues today's call
sequence and never touches the fused wrappers; on, one fused call per step and no `given=` pass, the loop completes, is reproducible per seed, differs
across seeds, draws inside the kept set of the step's own distribution and leaves the conditioning alone.  With the real kernels module a CPU tensor, or a
vocabulary the kernels refuse, keeps the tensor path."""
import os

import numpy as np
import pytest
import torch

import fake_kernels_nucleus as FK
from golden_utils import GOLDEN_DIR, Golden
from oracle import unidisc_oracle as O
from product_utils import build_product


def _golden():
    z = np.load(os.path.join(GOLDEN_DIR, "maskgit_nucleus_c_large.npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if z[k].dtype.kind != "U"}


class Spy:
    """the kernel doubles with every call to the row samplers recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(FK, name)
        if name in ("categorical_sample_rows", "nucleus_sample_rows", "ar_nucleus_rows", "nucleus_supported"):
            def wrapped(*a, **kw):
                self.calls.append((name, kw.get("given") is not None))
                return fn(*a, **kw)
            return wrapped
        return fn


def _product(monkeypatch, fused):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod
    from unidisc_amd.config import Cfg

    spy = Spy()
    monkeypatch.setattr(dit_mod, "K", spy)
    monkeypatch.setattr(diff_mod, "K", spy)
    g, s = Golden("c_large"), _golden()
    diff = build_product(g, device="cpu")
    diff.backbone.eval()
    kw = dict(maskgit_r_temp=float(s["r_temp"]), top_p=float(s["top_p"]), temperature=float(s["temperature"]))
    if fused is not None:
        kw["fused_nucleus"] = fused
    diff.config.eval = Cfg(**kw)
    return diff, spy, g, s


@pytest.mark.parametrize("fused", [None, False])
def test_key_off_keeps_todays_call_sequence(monkeypatch, fused):
    diff, spy, g, s = _product(monkeypatch, fused)
    steps = int(s["steps"])
    seen = []
    real = type(diff)._nucleus_draw
    monkeypatch.setattr(type(diff), "_nucleus_draw", lambda self, *a, **kw: (seen.append(1), real(self, *a, **kw))[1])
    x, nfe = diff.sample(num_steps=steps, batch_size=1, modality=s["modality"], predictor="maskgit_nucleus", seed=3, return_nfe=True)
    names = [c for c in spy.calls]
    assert names and all(n == ("categorical_sample_rows", True) for n in names[:-1]), names      # every step: _nucleus_draw, then the given= pass
    assert len(seen) == len([n for n in names if n == ("categorical_sample_rows", True)])
    assert not any(n[0] in ("nucleus_sample_rows", "ar_nucleus_rows", "nucleus_supported") for n in names)
    assert not (x == diff.mask_index).any()


def test_key_on_one_fused_call_per_step(monkeypatch):
    diff, spy, g, s = _product(monkeypatch, True)
    steps = int(s["steps"])
    monkeypatch.setattr(type(diff), "_nucleus_draw", lambda self, *a, **kw: pytest.fail("_nucleus_draw ran with eval.fused_nucleus on"))
    x0, x0_unmask, mod = s["x0"], s["x0_unmask"].bool(), s["modality"]
    B = 2
    run = lambda seed: diff.sample(num_steps=steps, x0=x0.expand(B, -1), x0_unmask=x0_unmask.expand(B, -1), batch_size=B, modality=mod.expand(B, -1).contiguous(),
                                   predictor="maskgit_nucleus", seed=seed, return_nfe=True)
    spy.calls.clear()
    a, nfe = run(3)
    fused = [c for c in spy.calls if c[0] == "nucleus_sample_rows"]
    assert len(fused) >= 2 and len(fused) == nfe - 1, (len(fused), nfe)                  # one fused call per maskgit step (the last evaluation is the noise removal)
    assert not any(c == ("categorical_sample_rows", True) for c in spy.calls), "a given= pass ran beside the fused call"
    assert not (a == diff.mask_index).any()
    assert torch.equal(a[x0_unmask.expand(B, -1)], x0.expand(B, -1)[x0_unmask.expand(B, -1)])       # conditioning positions untouched
    b, _ = run(3)
    c, _ = run(4)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_key_on_replayed_pred_still_goes_through_given(monkeypatch):
    """a replayed `pred` takes categorical_sample_rows(given=) with the key on as with it off: the two runs agree bit for bit"""
    outs = []
    for fused in (False, True):
        diff, spy, g, s = _product(monkeypatch, fused)
        steps = int(s["steps"])
        replay = [(s[f"step{i}/pred"], s[f"step{i}/gumbel"].float()) if f"step{i}/pred" in s else (None, None) for i in range(steps)]
        assert all(p is not None for p, _ in replay[:2])
        x, nfe = diff.sample(num_steps=steps, eps=float(s["eps"]), x0=s["x0"], x0_unmask=s["x0_unmask"].bool(), batch_size=1, modality=s["modality"],
                             predictor="maskgit_nucleus", replay=replay, seed=3, return_nfe=True)
        given = [c for c in spy.calls if c == ("categorical_sample_rows", True)]
        assert len(given) >= sum(1 for p, _ in replay if p is not None) - 1 and len(given) >= 2
        if all(p is not None for p, _ in replay):
            assert not any(c[0] == "nucleus_sample_rows" for c in spy.calls)
        outs.append((x, nfe))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_ar_double_follows_the_write_back_rules():
    """the double of udm_ar_nucleus_rows: x[r, pos], next_ids and the unconditional half's [MASK], as udm_ar_sample_rows"""
    R, V, Vt, mask_id, L, pos = 4, 64, 43, 40, 6, 2
    gen = torch.Generator().manual_seed(1)
    logits = torch.randn(2 * R, 72, generator=gen).bfloat16()
    x = torch.full((R, L), 7)
    x0 = torch.randint(0, V, (R, L), generator=gen)
    unmask = torch.zeros(R, L, dtype=torch.bool)
    unmask[1, pos] = True
    ids = torch.full((2 * R,), -1)
    mod = torch.zeros(R, L, dtype=torch.int64)
    mod[2:, pos] = 1
    FK.ar_nucleus_rows(logits, x, pos, V, Vt, mask_id, inv_temperature=1 / 0.9, budget=0.95, step=1, modality=mod, restrict=True, seed=2, x0=x0, x0_unmask=unmask,
                       next_ids=ids, logits_u=logits[R:], w=torch.full((4,), 1.5), rows=R)
    col = x[:, pos]
    assert int(col[1]) == int(x0[1, pos]) and bool((col[:2][[0]] < Vt).all()) and bool((col[2:] >= Vt).all()) and not bool((col == mask_id)[[0, 2, 3]].any())
    assert torch.equal(ids[:R], col) and int(ids[R + 1]) == mask_id and torch.equal(ids[R:][[0, 2, 3]], col[[0, 2, 3]])
    assert bool((x[:, [0, 1, 3, 4, 5]] == 7).all())


def test_fused_tokens_lie_in_the_oracle_nucleus(monkeypatch):
    """tests/test_sampler.py:367-374 on the fused path: a free step's tokens come from `oracle.nucleus_filter`'s kept set of the step's own distribution"""
    diff, spy, g, s = _product(monkeypatch, True)
    xs = s["step1/x"]
    t = s["timesteps"][1] * torch.ones(1, 1)
    sched = diff.adap_sche(xs, int(s["steps"]), diff.mask_index, "arccos")
    got = {}
    real = FK.nucleus_sample_rows

    def grab(logits, *a, **kw):
        out = real(logits, *a, **kw)
        got.update(logits=logits, tok=out[0], kw=kw)
        return out

    monkeypatch.setattr(FK, "nucleus_sample_rows", grab)
    diff._maskgit_nucleus_update(xs, t, None, schedule=sched, step=1, modality=s["modality"], seed=5)
    n = got["logits"].shape[0]
    assert got["kw"]["inv_temperature"] == 1.0 and abs(got["kw"]["budget"] - float(s["top_p"]) * float(s["temperature"])) < 1e-12
    rm = got["kw"]["modality"]
    lp = O.subs_parameterization(g.cfg, got["logits"][:, : g.cfg.vocab_size].float()[None], torch.full((1, n), g.cfg.mask_index), rm[None] if rm is not None else None,
                                 None).float()[0]
    fp = O.nucleus_filter(lp.exp(), float(s["top_p"]), float(s["temperature"]))
    assert bool((fp.gather(-1, got["tok"][:, None]) > 0).all())


def test_unsupported_cases_keep_the_tensor_path():
    from unidisc_amd import kernels as K

    z = torch.zeros(2, 72, dtype=torch.bfloat16)
    assert K.nucleus_supported(z, 64) is False                        # a CPU tensor
    assert K.NUCLEUS_V_MAX == 65536

    class OnGpu:                                                      # what the predicate looks at
        is_cuda, dtype = True, torch.bfloat16

    assert K.nucleus_supported(OnGpu(), 65536) is True and K.nucleus_supported(OnGpu(), 65537) is False
