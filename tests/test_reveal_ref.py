"""tests/reveal_ref.py, the exact CPU statement of `udm_reveal_rows` that every other reveal test compares against: it equals today's tensor statements
(`Diffusion._maskgit_reveal`, `Diffusion._first_hitting_reveal`) bit for bit on inputs with distinct noise, it reproduces every recorded step of the
reference's maskgit / maskgit_nucleus / first_hitting runs (no step excluded), and the comparison (torch.equal on x_out) tells it from every seeded mutant."""
import os

import numpy as np
import pytest
import torch

import reveal_ref as R
from golden_utils import GOLDEN_DIR, Golden
from oracle import unidisc_oracle as O

SHAPES = [(1, 1), (1, 37), (3, 5), (3, 37), (2, 130)]


def _kw(c):
    return {k: v for k, v in c.items() if k != "x"}


@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("family", ["random", "gap", "all_masked", "k0", "k1", "k_count", "k_above", "neg_inf", "t_one", "t_small"])
def test_equals_todays_maskgit_reveal(B, L, family):
    from unidisc_amd.diffusion import Diffusion

    for seed in range(3):
        c = R.make_case(B, L, False, family, seed=seed)
        x = c["x"]
        copy_flag = x != R.MASK
        conf = R.confidence(torch.zeros(B, L), c["noise"], c["t"], R.R_TEMP)[~copy_flag]
        assert conf.unique().numel() == conf.numel()                        # distinct noise: no tie for the tensor path to leave undefined
        k = torch.minimum(c["sched"], (~copy_flag).sum(-1))
        if bool((k <= 0).all()):                                            # the step's early exit: `_maskgit_update` returns x before the tail
            assert torch.equal(R.reveal_ref(x, R.MASK, **_kw(c)), x)
            continue
        got, _ = Diffusion._maskgit_reveal(None, x, copy_flag, k, c["rows"], c["tok"], c["logp"], c["noise"], 0, R.R_TEMP, c["t"][:, None])
        assert torch.equal(R.reveal_ref(x, R.MASK, **_kw(c)), got)


@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("family", ["random", "gap", "all_masked", "k0", "k1", "k_count", "k_above"])
def test_equals_todays_first_hitting_tail(B, L, family):
    from unidisc_amd.diffusion import Diffusion

    for seed in range(3):
        c = R.make_case(B, L, True, family, seed=seed)
        x = c["x"]
        copy_flag = x != R.MASK
        u = c["noise"][~copy_flag]
        assert u.unique().numel() == u.numel()
        k = torch.minimum(c["sched"], (~copy_flag).sum(-1))
        got = Diffusion._first_hitting_reveal(x, copy_flag, k, c["rows"], c["tok"], c["noise"], 0)
        assert torch.equal(R.reveal_ref(x, R.MASK, **_kw(c)), got)


def _load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if z[k].dtype.kind != "U"}


def golden_steps(fixture):
    """per recorded step of a sampler fixture: (operands of reveal_ref, step{i}/x_next).  log p and the first_hitting tokens come from the recorded logits
    through the oracle's SUBS parameterization, as in tests/test_sampler.py."""
    case = "b_small" if fixture.endswith("b_small") else "c_large"
    g, s = Golden(case), _load(fixture)
    cfg = g.cfg
    batch = O.update_batch(cfg, g.batch())
    modality = s["modality"] if "modality" in s else None
    lottery = fixture.startswith("first_hitting")
    x0, x0_unmask = (s["x0"], s["x0_unmask"].bool()) if "x0" in s else (None, None)
    for i in range(int(s["steps"])):
        x = s[f"step{i}/x"]
        B, L = x.shape
        kw = dict(sched=s["schedule"][:, i].to(torch.int64), lottery=lottery, x0=x0, x0_unmask=x0_unmask)
        rows = (x.reshape(-1) == cfg.mask_index).nonzero().reshape(-1)
        if f"step{i}/logits" in s and rows.numel():
            lp = O.subs_parameterization(cfg, s[f"step{i}/logits"].float(), x, modality, batch, bf16=False).float()
            if lottery:
                pred = O.sample_categorical(lp.exp(), s[f"step{i}/u"])
                kw.update(noise=s[f"step{i}/pos_u"].float())
            else:
                pred = s[f"step{i}/pred"]
                kw.update(noise=s[f"step{i}/gumbel"].float(), t=s["timesteps"][i] * torch.ones(B), r_temp=float(s["r_temp"]))
            tok = pred.reshape(-1)[rows]
            kw.update(rows=rows, tok=tok, logp=None if lottery else lp.reshape(B * L, -1)[rows].gather(-1, tok[:, None])[:, 0])
        else:
            kw.update(sched=None)
        yield i, x, cfg.mask_index, kw, s[f"step{i}/x_next"]


@pytest.mark.parametrize("fixture", ["maskgit_c_large", "maskgit_b_small", "maskgit_nucleus_c_large", "first_hitting_c_large", "first_hitting_b_small"])
def test_reproduces_the_recorded_reference_steps(fixture):
    seen = 0
    for i, x, mask, kw, want in golden_steps(fixture):
        got = R.reveal_ref(x, mask, **kw)
        assert torch.equal(got, want), f"step {i}: {int((got != want).sum())} positions differ"
        if kw["sched"] is not None:      # the premises the fixtures were checked for: every step reveals exactly its schedule count, no duplicate lottery value
            k = torch.minimum(kw["sched"], (x == mask).sum(-1))
            assert torch.equal(((x == mask) & (want != mask)).sum(-1), k), f"step {i}"
            if kw["lottery"]:
                assert all(r.unique().numel() == r.numel() for r in kw["noise"]), f"step {i}"
        seen += 1
    assert seen >= 4


CASES = {f"{'lottery' if lot else 'confidence'}:{name}": c for lot in (False, True) for name, c in R.all_cases(3, 37, lot).items()}


def _rejected(c, mutant):
    want = R.reveal_ref(c["x"], R.MASK, **_kw(c))
    try:
        return not torch.equal(R.reveal_ref(c["x"], R.MASK, mutant=mutant, **_kw(c)), want)
    except IndexError:                   # an unclamped k past the row
        return True


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_comparison_rejects_the_mutant(mutant):
    hits = [n for n, c in CASES.items() if _rejected(c, mutant)]
    assert hits, f"no case of the table tells {mutant} from the rule"
    expect = {"conf_fma": "confidence:fma_tie", "conf_order": "confidence:order_tie", "ties_desc_position": "lottery:dup_cut", "k_unclamped": "confidence:k_past_L",
              "writeback_first": "confidence:eos_in_x0", "first_eos_text_only": "lottery:eos_in_image", "pad_eos_itself": "confidence:eos_at_0",
              "pad_image": "lottery:eos_at_0", "pad_mask": "confidence:eos_at_0+k0", "strict_gt": "confidence:random", "k_plus_one": "lottery:random",
              "k_minus_one": "confidence:random"}
    assert expect[mutant] in hits, hits


def test_rule_is_deterministic_and_leaves_operands_alone():
    for name, c in CASES.items():
        before = {k: v.clone() for k, v in c.items() if isinstance(v, torch.Tensor)}
        a, b = R.reveal_ref(c["x"], R.MASK, **_kw(c)), R.reveal_ref(c["x"], R.MASK, **_kw(c))
        assert torch.equal(a, b), name
        assert all(torch.equal(v, c[k]) or (v.is_floating_point() and torch.equal(v.isnan(), c[k].isnan())) for k, v in before.items()), name
