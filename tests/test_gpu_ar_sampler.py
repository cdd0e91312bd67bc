"""The AR baseline's KV-cached sampler on the HIP path (`_ar_sampler`, model_eval.py:2736-2822; DIT.reset_kv_cache / forward(start_pos=...)).

Teacher forcing: decode step p gives row p of the full causal forward's logits - against the imported reference's fp32 logits (tests/golden/ar_*.npz,
1-D rope in ar_b_small, 2-D rope in ar_c_large) within the AR bound of tests/test_gpu_ar.py, and prefill + decode equals pure decode.  The sampler: every
argmax token is the argmax of (next-token logits + the given Gumbel noise) of its teacher-forced row wherever that row's top-two margin is not a near tie,
with and without guidance and conditioning; top-p tokens lie in the reference rule's nucleus; the token loop makes no host synchronisation."""
import types

import pytest
import torch

from ar_utils import ArGolden, ar_config, build_ar_product
from golden_utils import rel_err
from oracle.cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
NLL_BOUND = 4.5e-3
MARGIN_EPS = 0.05   # top-two margin below which the two bf16 paths (decode vs full forward) may order a pair differently


def floor_bound(floor):
    return max(1.25 * floor + 5e-4, NLL_BOUND)


def _eval_product(name):
    g = ArGolden(name)
    diff = build_ar_product(g, DEV)
    diff.backbone.eval()
    return g, diff


def _decode_all(bb, x, mod, n_prefill=1):
    """logits [B, L, V] of x by prefill (n_prefill tokens) + one decode step per later position"""
    B, L = x.shape
    bb.reset_kv_cache(batch_size=B, seq_len=L, dtype=torch.bfloat16, device=DEV, modality=mod)
    rows = [bb(x[:, :n_prefill], None, modality=mod[:, :n_prefill], start_pos=0).float()]
    for p in range(n_prefill, L):
        rows.append(bb(x[:, p:p + 1], None, modality=mod[:, p:p + 1], start_pos=p).float())
    out = torch.cat(rows, 1)
    bb.reset_kv_cache(set_to_none=True)
    return out


@pytest.mark.parametrize("name", ["ar_b_small", "ar_c_large"])
def test_decode_teacher_forced_matches_full_forward(name):
    g, diff = _eval_product(name)
    bb = diff.backbone
    x, mod = g.t("fp32/input_ids").to(DEV), g.t("fp32/modality").to(DEV)
    truth = g.t("fp32/logits")
    bound = floor_bound(rel_err(g.t("bf16/logits"), truth))
    with torch.no_grad():
        full = bb(x, None, modality=mod).float()
        dec = _decode_all(bb, x, mod, 1)
        dec8 = _decode_all(bb, x, mod, 8)
    assert rel_err(full.cpu(), truth) < bound
    assert rel_err(dec.cpu(), truth) < bound
    for p in range(x.shape[1]):
        assert rel_err(dec[:, p], full[:, p]) < 1e-2, p
    assert rel_err(dec8, dec) < 1e-2
    assert bb._kv is None


def _teacher_forced_next(diff, x, mod):
    """next-token logits [B, L, V] fp32 of the full causal forward on x"""
    with torch.no_grad():
        return diff.backbone(x, None, modality=mod).float()


def _excluded(diff, nxt_mod):
    V, Vt = diff.vocab_size, diff.text_vocab_size
    ids = torch.arange(V, device=DEV)
    return (ids == diff.mask_index)[None, None] | torch.where((nxt_mod == 1)[..., None], ids < Vt, ids >= Vt)


def _check_argmax_run(diff, x, nfe, noise, mod, z_of, x0=None, x0_unmask=None):
    B, L = x.shape
    assert nfe == L - 1
    z = z_of(x)[:, :-1] + noise                                   # [B, L-1, V]: row i chooses token i + 1
    z = z.masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
    top2 = z.topk(2, -1).values
    margin = top2[..., 0] - top2[..., 1]
    y = z.argmax(-1)
    if x0 is not None:
        y = torch.where(x0_unmask[:, 1:], x0[:, 1:], y)
    sure = margin > MARGIN_EPS
    assert sure.float().mean() > 0.9
    assert torch.equal(x[:, 1:][sure], y[sure])


def _ar_diff(seed=0, **case_kw):
    from unidisc_amd import Diffusion

    case = dict(CASES["c_large"], **case_kw)
    torch.manual_seed(seed)
    diff = Diffusion(ar_config(case), None, DEV)
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "embed" in n or "attn" in n or "mlp" in n:
                p.copy_((torch.randn(p.shape, generator=gen) * 2 / p.shape[-1] ** 0.5).to(DEV))
    diff.backbone.eval()
    return diff


def _static_mod(diff, B):
    L = diff.config.model.length
    mod = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    mod[:, diff.static_img_sl] = 1
    return mod


@pytest.mark.parametrize("cond", [False, True])
def test_sampler_argmax_replays_noise(cond):
    diff = _ar_diff(1)
    B, L, V = 4, diff.config.model.length, diff.vocab_size
    mod = _static_mod(diff, B)
    gen = torch.Generator().manual_seed(11)
    noise = -torch.log(-torch.log(torch.rand(B, L - 1, V, generator=gen).clamp(1e-10, 1 - 1e-7))).to(DEV)
    x0 = x0_unmask = None
    if cond:
        x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to(DEV)
        x0_unmask = torch.zeros(B, L, dtype=torch.bool, device=DEV)
        x0_unmask[:, :diff.config.model.txt_length] = True
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, noise=noise, bos_token_id=3)
    assert x.shape == (B, L) and (x[:, 0] == (x0[:, 0] if cond else 3)).all()
    if cond:
        assert torch.equal(x[x0_unmask], x0[x0_unmask])
    assert not (x == diff.mask_index).any()
    _check_argmax_run(diff, x, nfe, noise, mod, lambda xx: _teacher_forced_next(diff, xx, mod), x0, x0_unmask)
    x2, _ = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, noise=noise, bos_token_id=3)
    assert torch.equal(x, x2)
    # Philox noise: deterministic per seed
    xa, _ = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=7, bos_token_id=3)
    xb, _ = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=7, bos_token_id=3)
    assert torch.equal(xa, xb)


def test_sampler_cfg_replays_noise():
    diff = _ar_diff(2)
    diff.config.eval.cfg = 1.5
    diff.config.eval.force_cfg_value = True
    B, L, V = 4, diff.config.model.length, diff.vocab_size
    mod = _static_mod(diff, B)
    gen = torch.Generator().manual_seed(12)
    noise = -torch.log(-torch.log(torch.rand(B, L - 1, V, generator=gen).clamp(1e-10, 1 - 1e-7))).to(DEV)
    x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to(DEV)
    x0_unmask = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    x0_unmask[:, :diff.config.model.txt_length] = True
    diff.tokenizer = types.SimpleNamespace(bos_token_id=3)   # (through sample(): the BOS id comes from the tokenizer)
    x, nfe = diff.sample(x0=x0, x0_unmask=x0_unmask, modality=mod, noise=noise, return_nfe=True)

    def z_of(xx):
        xu = torch.where(x0_unmask, diff.mask_index, xx)
        return 2.5 * _teacher_forced_next(diff, xx, mod) - 1.5 * _teacher_forced_next(diff, xu, mod)

    assert torch.equal(x[x0_unmask], x0[x0_unmask])
    _check_argmax_run(diff, x, nfe, noise, mod, z_of, x0, x0_unmask)
    diff.config.eval.force_cfg_value = False
    with pytest.raises(NotImplementedError, match="force_cfg_value"):
        diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, bos_token_id=3)


def test_sampler_top_p_draws_from_the_nucleus():
    diff = _ar_diff(3)
    diff.config.eval.top_p = 0.8
    diff.config.eval.temperature = 0.7
    B, L = 8, diff.config.model.length
    mod = _static_mod(diff, B)
    x, nfe = diff._ar_sampler(B, modality=mod, seed=5, bos_token_id=3)
    assert nfe == 0
    z = _teacher_forced_next(diff, x, mod)[:, :-1].masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
    probs = torch.softmax(z / 0.7, -1)
    p_tok = probs.gather(-1, x[:, 1:, None])[..., 0]
    mass_above = (probs * (probs > p_tok[..., None])).sum(-1)      # probability of the ids ranked above the drawn one
    top = probs.max(-1).values
    # (the drawn id's nucleus test on the full forward's logits: the decode path's bf16 logits move a boundary id's cumulative mass by a few 1e-2 at T = 0.7)
    in_nucleus = (mass_above + p_tok <= 0.8 + 5e-2) | (p_tok >= top - 1e-4)
    assert in_nucleus.all(), (mass_above + p_tok)[~in_nucleus]


@pytest.mark.parametrize("cond", [False, True])
def test_sampler_has_no_host_sync_and_frees_cache(cond):
    """Diffusion._ar_sampler itself under torch.cuda.set_sync_debug_mode("error").  Conditioned, the one host read of the run - the length of the
    fixed prefix, before the token loop - is taken outside (the same value) so that the rest of the run, the loop included, is checked."""
    diff = _ar_diff(4)
    B, L = 4, diff.config.model.length
    mod = _static_mod(diff, B)
    x0 = x0_unmask = None
    if cond:
        gen = torch.Generator().manual_seed(4)
        x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen).to(DEV)
        x0_unmask = torch.zeros(B, L, dtype=torch.bool, device=DEV)
        x0_unmask[:, :diff.config.model.txt_length] = True
        n0 = type(diff)._ar_fixed_prefix(x0_unmask, L)
        diff._ar_fixed_prefix = lambda u, LL: n0
    diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=9, bos_token_id=3)   # (warm-up: first launches, allocator)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=mod, seed=9, bos_token_id=3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert nfe == L - 1 and not (x[:, 1:] == diff.mask_index).any()
    assert diff.backbone._kv is None    # the sampler frees its cache (reset_kv_cache(set_to_none=True))
    bb = diff.backbone
    bb.reset_kv_cache(batch_size=B, seq_len=L - 1, dtype=torch.bfloat16, device=DEV, modality=mod)
    assert bb._kv is not None and len(bb._kv.K) == bb.n_blocks
    bb.reset_kv_cache(set_to_none=True)
    assert bb._kv is None
