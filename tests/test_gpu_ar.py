"""The AR baseline end to end on the HIP path (parameterization=ar, trainer.ar_shift, model.full_attention=false; configs/experiments/ar.yaml):
against the imported reference's AR goldens (tests/golden/ar_*.npz, scripts/make_golden_ar.py), against torch fp32 on the engine's own logits at
UniDisc-S width, and on the properties the causal model must have - causality bit for bit, gradient checkpointing bit for bit, no RNG use.

Bounds, in the style of tests/test_gpu_e2e.py (tied to the reference's own bf16-vs-fp32 floor): loss 1e-3 relative; log p and logits rel-RMS
1.25 x the reference's bf16 deviation + 5e-4 (floored at the SUBS per-token NLL bound, 4.5e-3); per-parameter gradients 6e-2 (worst) / 3e-2 (median)."""
import pytest
import torch

from ar_utils import AR_CASE_NAMES, ArGolden, ar_config, build_ar_product
from golden_utils import rel_err
from oracle.cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_BOUND, NLL_BOUND, GRAD_BOUND = 1e-3, 4.5e-3, 6e-2


def floor_bound(floor):
    return max(1.25 * floor + 5e-4, NLL_BOUND)


@pytest.mark.parametrize("name", AR_CASE_NAMES)
def test_ar_step_matches_golden(name):
    g = ArGolden(name)
    diff = build_ar_product(g, DEV)
    rng = torch.cuda.get_rng_state()
    out = diff.training_step(g.batch(), 1)
    assert torch.equal(torch.cuda.get_rng_state(), rng)   # AR draws nothing: no t, no corruption
    assert torch.equal(out.token_mask.cpu(), g.t("fp32/token_mask"))
    l32 = float(g.t("fp32/loss"))
    assert abs(float(out.loss.detach()) - l32) / abs(l32) < LOSS_BOUND
    lp, lp32 = diff._last["log_p_theta"].float().cpu(), g.t("fp32/log_p")
    assert lp.shape == lp32.shape
    assert rel_err(lp, lp32) < floor_bound(rel_err(g.t("bf16/log_p"), lp32))
    assert rel_err(out.nlls.cpu(), g.t("fp32/nlls")) < floor_bound(rel_err(g.t("bf16/nlls"), g.t("fp32/nlls")))
    for k in ("txt_loss", "img_loss"):
        if g.has("fp32/" + k):
            v32 = float(g.t("fp32/" + k))
            assert abs(float(getattr(out, k)) - v32) / max(abs(v32), 1e-6) < 3 * LOSS_BOUND, k
    with torch.no_grad():
        logits = diff.backbone(g.t("fp32/input_ids").to(DEV), None, modality=g.t("fp32/modality").to(DEV))
    truth = g.t("fp32/logits")
    assert rel_err(logits.float().cpu(), truth) < floor_bound(rel_err(g.t("bf16/logits"), truth))
    out.loss.backward()
    torch.cuda.synchronize()
    named = dict(diff.backbone.named_parameters())
    gref = g.grads()
    assert set(gref) == {k for k, p in named.items() if p.grad is not None}
    errs = sorted(((rel_err(named[k].grad.cpu(), gr), k) for k, gr in gref.items()), reverse=True)
    assert errs[0][0] < GRAD_BOUND, errs[0]
    assert errs[len(errs) // 2][0] < GRAD_BOUND / 2, errs[len(errs) // 2]


def _ar_product(case, seed=0):
    from unidisc_amd import Diffusion

    torch.manual_seed(seed)
    diff = Diffusion(ar_config(case), None, DEV)
    diff.backbone.train()
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "embed" in n:
                p.copy_((torch.randn(p.shape, generator=gen) / p.shape[-1] ** 0.5).to(DEV))
    return diff


def _token_batch(B, Lt, Li, Vt, Vi, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(txt_input_ids=torch.randint(0, Vt - 1, (B, Lt), generator=gen, dtype=torch.int32),
                img_input_ids=torch.randint(0, Vi, (B, Li), generator=gen, dtype=torch.int32).to(torch.int16),
                txt_attention_mask=torch.ones(B, Lt, dtype=torch.bool))


def test_ar_at_unidisc_s_width_matches_torch_on_own_logits():
    """12 blocks, d = 768, V = 40 193: the fused AR loss and log p against torch fp32 on the engine's own bf16 logits (logits[:, :-1], the [MASK] column
    and the other modality than the target's excluded, log-softmax, gather x0[:, 1:], masked mean)."""
    case = dict(CASES["b_small"], hidden_size=768, n_heads=12, cond_dim=128, n_blocks=12, batch_size=64, txt_length=128, img_length=128, text_vocab_size=32001,
                vocab_size=40193, text_loss_weight=None, force_full_attention_mask_loss_only=None)
    diff = _ar_product(case)
    # B = 64: B (L - 1) head rows leave whole 64-row groups out, so the head is compacted (and split by the targets' modality) as at UniDisc-S
    batch = _token_batch(64, 128, 128, 32001, 8192, 1)
    out = diff.training_step(batch, 1)
    lp = diff._last["log_p_theta"].float()
    x0, mod = diff._last["xt"], diff._last["modality"]
    with torch.no_grad():
        logits = diff.backbone(x0, None, modality=mod)[:, :-1].float()
    V, Vt = diff.vocab_size, diff.text_vocab_size
    cols = torch.arange(V, device=DEV)
    tgt_img = (mod[:, 1:] == 1)[..., None]
    bad = (cols == diff.mask_index) | torch.where(tgt_img, cols < Vt, cols >= Vt)
    ref = torch.cat([torch.log_softmax(lg.masked_fill(bd, float("-inf")), -1).gather(-1, t[..., None])[..., 0]   # (8 rows at a time: [64, 255, V] fp32 is 2.6 GB)
                     for lg, bd, t in zip(logits.split(8), bad.split(8), x0[:, 1:].split(8))])
    assert torch.isfinite(lp).all()
    assert rel_err(lp, ref) < 1e-3 and float((lp - ref).abs().max()) < 2e-2
    am = out.token_mask.float()
    loss_ref = float((-ref * am).sum() / am.sum())
    assert abs(float(out.loss.detach()) - loss_ref) / loss_ref < 1e-4
    out.loss.backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in diff.backbone.parameters() if p.grad is not None)


def _small_long_case():
    return dict(CASES["b_small"], batch_size=2, txt_length=128, img_length=128, ragged_text=False, text_loss_weight=None, force_full_attention_mask_loss_only=None)


def test_ar_is_causal_end_to_end():
    """Changing token p changes no log p of a row before p - 1 (row r predicts token r + 1 from tokens <= r), bit for bit.  (p a multiple of 32: the
    attention forward's lazy rescale is decided per wave of 32 query rows, see tests/test_gpu_attention_causal.py.)"""
    case = _small_long_case()
    diff = _ar_product(case, seed=3)
    batch = _token_batch(2, 128, 128, case["text_vocab_size"], case["vocab_size"] - case["text_vocab_size"], 2)
    with torch.no_grad():
        diff.training_step({k: v.clone() for k, v in batch.items()}, 1)
        lp0 = diff._last["log_p_theta"].clone()
        for p in (64, 160):
            b2 = {k: v.clone() for k, v in batch.items()}
            if p < 128:
                b2["txt_input_ids"][:, p] = (b2["txt_input_ids"][:, p] + 7) % (case["text_vocab_size"] - 1)
            else:
                b2["img_input_ids"][:, p - 128] = (b2["img_input_ids"][:, p - 128] + 7) % (case["vocab_size"] - case["text_vocab_size"])
            diff.training_step(b2, 1)
            lp = diff._last["log_p_theta"]
            assert torch.equal(lp[:, : p - 1], lp0[:, : p - 1]), p
            assert not torch.equal(lp[:, p - 1:], lp0[:, p - 1:]), p


def test_ar_gradient_checkpointing_is_bit_identical():
    """trainer.use_gradient_checkpointing in AR mode: every block re-run from its saved input with the same causal flag.  Loss and log p bit for bit; the
    weight gradients of the Linears (written whole by their wgrad kernels) bit for bit; the vectors and embeddings the backward accumulates with fp32
    atomics within their run-to-run noise (the bound of tests/test_gpu_e2e.py: two runs WITHOUT checkpointing differ there in the same way)."""
    g = ArGolden("ar_c_large")
    res = []
    for ckpt in (False, True):
        diff = build_ar_product(g, DEV)
        diff.backbone.use_gradient_checkpointing = ckpt
        out = diff.training_step(g.batch(), 1)
        out.loss.backward()
        torch.cuda.synchronize()
        res.append((out.loss.detach().clone(), diff._last["log_p_theta"].detach().clone(),
                    {k: p.grad.clone() for k, p in diff.backbone.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    g0, g1 = res[0][2], res[1][2]
    assert g0.keys() == g1.keys()
    lin = [k for k in g0 if g0[k].dim() == 2 and "embed" not in k]
    assert lin
    for k in g0:
        if k in lin:
            assert torch.equal(g0[k], g1[k]), k
        else:
            assert rel_err(g1[k].cpu(), g0[k].cpu()) < 2e-3, k


def test_ar_forward_log_probs():
    g = ArGolden("ar_c_large")
    diff = build_ar_product(g, DEV)
    diff.backbone.eval()
    x, mod = g.t("fp32/input_ids").to(DEV), g.t("fp32/modality").to(DEV)
    B, L = x.shape
    V, Vt = diff.vocab_size, diff.text_vocab_size
    with torch.no_grad():
        lp = diff.forward(x, None, modality=mod).float()
        lp_full = diff.forward(x, None, modality=mod, disable_ar_shift=True).float()
    assert lp.shape == (B, L - 1, V) and lp_full.shape == (B, L, V)
    ninf = lp <= -1e5   # excluded ids: the reference's finite neg_infinity (-1e6)
    tgt_img = (mod[:, 1:] == 1)[..., None]
    cols = torch.arange(V, device=DEV)
    expect = (cols == diff.mask_index) | torch.where(tgt_img, cols < Vt, cols >= Vt)
    assert torch.equal(ninf, expect.expand_as(ninf))
    assert torch.equal(lp_full <= -1e5, (cols == diff.mask_index).expand(B, L, V))   # unshifted: the [MASK] column only (model.py:760)
    assert torch.allclose(torch.logsumexp(lp, -1), torch.zeros(B, L - 1, device=DEV), atol=1e-2)
    truth = g.t("fp32/log_p")
    got = lp.gather(-1, x[:, 1:, None])[..., 0].cpu()
    assert rel_err(got, truth) < floor_bound(rel_err(g.t("bf16/log_p"), truth)) + 4e-3   # (bf16 log-probs: one more rounding than the fused path)
