"""The AR sampler against the reference's OWN `_ar_sampler` (model_eval.py:2736-2822): fixtures tests/golden/ar_sampler_{uncond,cond,cfg}.npz made by
scripts/make_golden_ar_sampler.py on b_small's AR parameters (those of ar_b_small.npz), with the reference's Gumbel draw, final tokens, nfe, and per step its
fp32 `next` row and the margin between the top two values of next + noise.

- The product's next-token distribution of every step, teacher-forced on the reference's tokens, equals the reference's `next` up to a per-row constant
  (log-softmax over the admissible ids) within a bf16 bound, and the set of excluded ids ([MASK], the other modality than the NEXT position's) is the same.
- The product's token of every step (its own kernel on its own decode logits with the recorded noise) equals the reference's wherever the recorded margin
  exceeds EPS (the distance a bf16 path can move a score: 0.05 per unit of guidance scale (1 + 2 w)).
- Free-running with the recorded noise, each row's tokens equal the reference's up to that row's first step with a margin below EPS; nfe matches."""
import os

import numpy as np
import pytest
import torch

from ar_utils import ArGolden, build_ar_product
from golden_utils import rel_err
from unidisc_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = ["uncond", "cond", "cfg"]


def _fixture(run):
    z = np.load(os.path.join(GOLDEN_DIR, f"ar_sampler_{run}.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("meta/")}


def _product(f):
    diff = build_ar_product(ArGolden("ar_b_small"), DEV)
    diff.backbone.eval()
    if "cfg" in f:
        diff.config.eval.cfg = float(f["cfg"])
        diff.config.eval.force_cfg_value = True
    return diff


def _eps(f):
    w = float(f["cfg"]) if "cfg" in f else 0.0
    return 0.05 * (1 + 2 * w)


@pytest.mark.parametrize("run", RUNS)
def test_teacher_forced_steps_match_reference(run):
    f = _fixture(run)
    diff = _product(f)
    bb = diff.backbone
    x_ref, mod, noise = f["x"].to(DEV), f["modality"].to(DEV), f["noise"].to(DEV)
    B, L = x_ref.shape
    V = diff.vocab_size
    guided = "cfg" in f
    x0 = f["x0"].to(DEV) if "x0" in f else None
    unmask = f["x0_unmask"].to(DEV) if "x0_unmask" in f else None
    R = 2 * B if guided else B
    w = float(f["cfg"]) if guided else 0.0
    ids = x_ref if not guided else torch.cat([x_ref, torch.where(unmask, diff.mask_index, x_ref)], 0)
    mods = mod if not guided else torch.cat([mod, mod], 0)
    bb.reset_kv_cache(batch_size=R, seq_len=L - 1, dtype=torch.bfloat16, device=DEV, modality=mods)
    kv = bb._kv
    wt = torch.full((4,), w, device=DEV)
    nxt, toks = [], []
    with torch.no_grad():
        bb._prefill(ids[:, :1], mods[:, :1], last_only=True)
        for i in range(L - 1):
            if i > 0:
                kv.ids[:R] = ids[:, i]
                bb._decode_step(i)
            lg = kv.logits[:, :V].float()
            nxt.append(((1 + w) * lg[:B] - w * lg[B:2 * B]) if guided else lg[:B])
            xs = torch.zeros(B, L, dtype=torch.int64, device=DEV)
            K.ar_sample_rows(kv.logits, xs, i + 1, V, diff.text_vocab_size, diff.mask_index, step=i, modality=mod, restrict=True, g=noise, g_col0=i * V,
                             logits_u=kv.logits[B:] if guided else None, w=wt if guided else None, rows=B)
            toks.append(xs[:, i + 1].clone())
    bb.reset_kv_cache(set_to_none=True)
    nxt, toks = torch.stack(nxt, 1), torch.stack(toks, 1)                    # [B, L-1, V], [B, L-1]
    ref_next = f["next"].to(DEV)
    bad_ref = ref_next < -1e5                                                 # the reference's excluded ids ([MASK] at -1e6, the restriction at finfo.min)
    assert bad_ref.any(-1).all()
    # the product's excluded set, rebuilt from the rule the kernel applies, must be the reference's
    ids_v = torch.arange(V, device=DEV)
    img = (mod[:, 1:] == 1)[..., None]
    bad = (ids_v == diff.mask_index) | torch.where(img, ids_v < diff.text_vocab_size, ids_v >= diff.text_vocab_size)
    assert torch.equal(bad, bad_ref)
    lp = torch.log_softmax(nxt.masked_fill(bad, float("-inf")), -1)
    lr = torch.log_softmax(ref_next.masked_fill(bad_ref, float("-inf")), -1)
    assert rel_err(lp[~bad], lr[~bad]) < 1e-2 * (1 + 2 * w)
    sure = f["margin"].to(DEV) > _eps(f)
    assert sure.float().mean() > 0.85
    # the reference's token of step i is x[:, i+1] after its x0 write-back: compare where nothing overwrote the draw
    free = ~unmask[:, 1:] if unmask is not None else torch.ones_like(sure)
    chk = sure & free
    assert chk.any()
    assert torch.equal(toks[chk], x_ref[:, 1:][chk])


@pytest.mark.parametrize("run", RUNS)
def test_free_running_matches_reference(run):
    f = _fixture(run)
    diff = _product(f)
    x_ref, mod, noise = f["x"].to(DEV), f["modality"].to(DEV), f["noise"].to(DEV)
    B, L = x_ref.shape
    x0 = f["x0"].to(DEV) if "x0" in f else None
    unmask = f["x0_unmask"].to(DEV) if "x0_unmask" in f else None
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, noise=noise, bos_token_id=int(f["bos"]))
    assert nfe == int(f["nfe"])
    if unmask is not None:
        assert torch.equal(x[unmask], x0[unmask])
    low = (f["margin"].to(DEV) <= _eps(f))
    if unmask is not None:
        low &= ~unmask[:, 1:]                                                # (a near tie whose draw x0 overwrites decides nothing)
    agreed = 0
    for b in range(B):
        first = int(low[b].nonzero()[0]) if low[b].any() else L - 1        # steps 0..first-1 are certain: tokens 1..first
        assert torch.equal(x[b, :first + 1], x_ref[b, :first + 1]), (b, first)
        agreed += first
    assert agreed >= 4 * B   # (not vacuous: the unconditional fixture has near ties early in some rows; 26 of its 124 steps precede them)
