"""The KV-cached AR sampler at 65 .. 128 cache rows (batch 64 with guidance is 128 rows on one cache): DIT.reset_kv_cache, the decode step and the sampler
around it, on the tiny AR products of tests/test_gpu_ar_sampler.py whose helpers and rules are used as they stand.

1. reset_kv_cache allocates 65 (padded to 72), 72 and 128 rows and refuses 129.
2. Teacher forcing at 72 and at 128 rows: decode step p gives row p of the full causal forward of the same product (rel 1e-2 at every position), and a
   prefill of 8 tokens + decode is within 1e-2 of pure decode; 1-D rope (ar_b_small) and 2-D rope (ar_c_large).  Every row has its own tokens.
3. K.attention_decode and K.attention_decode_at at (B, H) = (72, 2) and (128, 16) - B H = 2048 plans one split, grid (B H, 1) - against torch fp32 with the
   bounds of tests/test_gpu_ar_decode_kernels.py; every cache slot but p unchanged bit for bit; the device-position form bit-identical.
4. The sampler at 72 unguided rows and at 40 guided samples (80 cache rows) with recorded Gumbel noise: _check_argmax_run (every token is the argmax of
   teacher-forced logits + noise where the top-two margin exceeds 0.05, more than 90 % of the positions sure), given positions equal x0, a second call
   returns equal tokens, Philox with one seed is deterministic.
5. The modes at 72 rows: eval.ar_decode_graph on equals off, eval.ar_chunk_given with a given run in the middle, eval.fused_nucleus, no synchronising
   call in the token loop, the cache freed afterwards."""
import functools
import math
import types

import pytest
import torch

from golden_utils import rel_err
from test_gpu_ar_sampler import (_ar_diff, _check_argmax_run, _decode_all, _eval_product, _excluded, _static_mod, _teacher_forced_next)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


# ------------------------------------------------------------------------------------------------ 1. allocation
def test_cache_allocation_up_to_128_rows(K):
    diff = _ar_diff(0)
    bb = diff.backbone
    L = diff.config.model.length
    for n, Bp in ((65, 72), (72, 72), (128, 128)):
        bb.reset_kv_cache(batch_size=n, seq_len=L - 1, dtype=BF16, device=DEV, modality=_static_mod(diff, n))
        kv = bb._kv
        assert (kv.B, kv.Bp) == (n, Bp) and kv.K[0].shape[0] == Bp and kv.logits.shape[0] == Bp and kv.ids.numel() == Bp
        d = bb.hidden_size
        assert kv.gws.numel() >= max(K.skinny_ws_elems(Bp, N, Kd) for N, Kd in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d), (bb.vocab_size, d)))
        bb.reset_kv_cache(set_to_none=True)
    with pytest.raises(NotImplementedError, match="128"):
        bb.reset_kv_cache(batch_size=129, seq_len=L - 1, dtype=BF16, device=DEV, modality=_static_mod(diff, 129))
    assert bb._kv is None


# ------------------------------------------------------------------------------------------------ 2. teacher forcing
def _rows_of(g, diff, B):
    """B rows of the golden's geometry, each with its own tokens: the golden's modality row, text ids at text positions and image ids at image positions"""
    mod0 = g.t("fp32/modality")[:1]
    mod = mod0.expand(B, -1).contiguous().to(DEV)
    gen = torch.Generator().manual_seed(B)
    Vt, V = diff.text_vocab_size, diff.vocab_size
    txt = torch.randint(0, Vt - 1, mod.shape, generator=gen).to(DEV)
    img = torch.randint(Vt, V - 1, mod.shape, generator=gen).to(DEV)
    return torch.where(mod == 1, img, txt), mod


@pytest.mark.parametrize("B", [72, 128])
@pytest.mark.parametrize("name", ["ar_b_small", "ar_c_large"])
def test_decode_teacher_forced_matches_full_forward(name, B):
    g, diff = _eval_product(name)
    bb = diff.backbone
    x, mod = _rows_of(g, diff, B)
    with torch.no_grad():
        full = bb(x, None, modality=mod).float()
        dec = _decode_all(bb, x, mod, 1)
        dec8 = _decode_all(bb, x, mod, 8)
    assert dec.shape == full.shape and bool(torch.isfinite(dec).all())
    for p in range(x.shape[1]):
        assert rel_err(dec[:, p], full[:, p]) < 1e-2, p
    for r in (0, 63, 64, B - 1):      # (not only on average over the rows: the first and last row of each row group)
        assert rel_err(dec[r], full[r]) < 1e-2, r
    assert rel_err(dec8, dec) < 1e-2
    assert bb._kv is None


# ------------------------------------------------------------------------------------------------ 3. decode attention
D, LMAX = 64, 1024


@functools.lru_cache(maxsize=1)
def _caches(B, H):
    """sentinel content everywhere, shared by the positions of a (B, H) and never modified (every case works on clones)"""
    gen = torch.Generator(device=DEV).manual_seed(B * 131 + H)
    return tuple(torch.randn((B, LMAX, H * D), generator=gen, device=DEV, dtype=torch.float32).to(BF16) for _ in range(2))


@pytest.mark.parametrize("p", [0, 64, 65, 1000])
@pytest.mark.parametrize("B,H", [(72, 2), (128, 16)])
def test_attention_decode_rows(K, B, H, p):
    K0, V0 = _caches(B, H)
    d = H * D
    gen = torch.Generator().manual_seed(p * 7 + B)
    q = (torch.randn(B, d, generator=gen) * K.attention_q_scale(D)).to(BF16).to(DEV)
    qkr = torch.empty(B, 2 * d, dtype=BF16, device=DEV)          # (the engine's operand layout: q | k rows of qkr, v in qkv[:, 2d:])
    qkr[:, :d] = q
    qkr[:, d:] = torch.randn(B, d, generator=gen).to(BF16).to(DEV)
    qkv = torch.randn(B, 3 * d, generator=gen).to(BF16).to(DEV)
    ws = K.attention_decode_ws(B, H, D, DEV)
    Kc, Vc = K0.clone(), V0.clone()
    o = K.attention_decode(qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], Kc, Vc, p, H, D, ws=ws)
    Ka, Va = K0.clone(), V0.clone()
    pos_dev = torch.full((1,), p, dtype=torch.int64, device=DEV)
    ws.fill_(float("nan"))
    oa = K.attention_decode_at(qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], Ka, Va, pos_dev, H, D, ws=ws)
    torch.cuda.synchronize()
    keep = torch.ones(LMAX, dtype=torch.bool, device=DEV)
    keep[p] = False
    assert torch.equal(Kc[:, keep], K0[:, keep]) and torch.equal(Vc[:, keep], V0[:, keep])
    assert torch.equal(Kc[:, p], qkr[:, d:]) and torch.equal(Vc[:, p], qkv[:, 2 * d:])
    assert torch.equal(oa, o) and torch.equal(Ka, Kc) and torch.equal(Va, Vc)
    k = Kc[:, :p + 1].float().view(B, p + 1, H, D)
    v = Vc[:, :p + 1].float().view(B, p + 1, H, D)
    s = torch.einsum("bhd,blhd->bhl", q.float().view(B, H, D), k) * math.log(2.0)   # q holds q log2(e) / sqrt(D): base-2 scores
    ref = torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), v).reshape(B, d)
    assert rel_err(o.float(), ref) < 8e-3
    assert float((o.float() - ref).abs().max()) < 2e-2


# ------------------------------------------------------------------------------------------------ 4. the sampler
def _noise(B, L, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return -torch.log(-torch.log(torch.rand(B, L - 1, V, generator=gen).clamp(1e-10, 1 - 1e-7))).to(DEV)


def _text_given(diff, B, seed, run=None):
    """x0 / x0_unmask: the text prefix given in every row, optionally a run of columns [run[0], run[1]) given in every row as well"""
    L, Lt = diff.config.model.length, diff.config.model.txt_length
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen)
    x0[:, Lt:] = torch.randint(diff.text_vocab_size, diff.vocab_size - 1, (B, L - Lt), generator=gen)      # image ids at image positions
    unmask = torch.zeros(B, L, dtype=torch.bool)
    unmask[:, :Lt] = True
    if run is not None:
        unmask[:, run[0]:run[1]] = True
    return x0.to(DEV), unmask.to(DEV)


def test_sampler_72_rows_replays_noise():
    diff = _ar_diff(1)
    B, L, V = 72, diff.config.model.length, diff.vocab_size
    mod = _static_mod(diff, B)
    noise = _noise(B, L, V, 11)
    x, nfe = diff._ar_sampler(B, modality=mod, noise=noise, bos_token_id=3)
    assert x.shape == (B, L) and (x[:, 0] == 3).all() and not (x == diff.mask_index).any()
    _check_argmax_run(diff, x, nfe, noise, mod, lambda xx: _teacher_forced_next(diff, xx, mod))
    x2, _ = diff._ar_sampler(B, modality=mod, noise=noise, bos_token_id=3)
    assert torch.equal(x, x2)
    xa, _ = diff._ar_sampler(B, modality=mod, seed=7, bos_token_id=3)
    xb, _ = diff._ar_sampler(B, modality=mod, seed=7, bos_token_id=3)
    assert torch.equal(xa, xb)
    assert len({tuple(r) for r in xa.tolist()}) > B // 2      # (the rows draw their own noise)


def test_sampler_40_guided_samples_replay_noise():
    diff = _ar_diff(2)
    diff.config.eval.cfg = 1.5
    diff.config.eval.force_cfg_value = True
    diff.tokenizer = types.SimpleNamespace(bos_token_id=3)      # (through sample(): the BOS id comes from the tokenizer)
    B, L, V = 40, diff.config.model.length, diff.vocab_size
    mod = _static_mod(diff, B)
    noise = _noise(B, L, V, 12)
    x0, unmask = _text_given(diff, B, 12)
    x, nfe = diff.sample(x0=x0, x0_unmask=unmask, modality=mod, noise=noise, return_nfe=True)

    def z_of(xx):
        xu = torch.where(unmask, diff.mask_index, xx)
        return 2.5 * _teacher_forced_next(diff, xx, mod) - 1.5 * _teacher_forced_next(diff, xu, mod)

    assert torch.equal(x[unmask], x0[unmask])
    _check_argmax_run(diff, x, nfe, noise, mod, z_of, x0, unmask)
    x2 = diff.sample(x0=x0, x0_unmask=unmask, modality=mod, noise=noise)
    assert torch.equal(x, x2)
    xa = diff.sample(x0=x0, x0_unmask=unmask, modality=mod, seed=7)
    xb = diff.sample(x0=x0, x0_unmask=unmask, modality=mod, seed=7)
    assert torch.equal(xa, xb)
    assert diff.backbone._kv is None


# ------------------------------------------------------------------------------------------------ 5. the modes at 72 rows
def test_decode_graph_on_equals_off_at_72_rows():
    diff = _ar_diff(3)
    diff.tokenizer = types.SimpleNamespace(bos_token_id=3)
    B, L = 72, diff.config.model.length
    mod = _static_mod(diff, B)
    diff.config.eval.ar_decode_graph = False
    x_off = diff.sample(batch_size=B, modality=mod, seed=7)
    assert diff.ar_decode_stats == dict(captures=0, replays=0, eager_steps=L - 2, chunks=0)
    diff.config.eval.ar_decode_graph = True
    x_on = diff.sample(batch_size=B, modality=mod, seed=7)
    torch.cuda.synchronize()
    assert diff.ar_decode_stats == dict(captures=1, replays=L - 2, eager_steps=0, chunks=0)
    assert torch.equal(x_on, x_off) and not (x_on[:, 1:] == diff.mask_index).any()
    assert diff.backbone._kv is None


def test_chunk_given_run_in_the_middle_at_72_rows():
    diff = _ar_diff(6)
    diff.config.eval.ar_chunk_given = True
    diff.config.eval.ar_chunk_min_tokens = 2
    B, L, V = 72, diff.config.model.length, diff.vocab_size
    assert (L, diff.config.model.txt_length) == (32, 16)
    mod = _static_mod(diff, B)
    x0, unmask = _text_given(diff, B, 21, run=(18, 22))      # columns 18 .. 21 in every row: step 17 feeds the positions 17 .. 21
    noise = _noise(B, L, V, 13)
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, noise=noise, bos_token_id=3)
    assert diff.ar_decode_stats == dict(captures=0, replays=0, eager_steps=L - 1 - 16 - 5, chunks=1)
    assert torch.equal(x[unmask], x0[unmask]) and not (x == diff.mask_index).any()
    _check_argmax_run(diff, x, nfe, noise, mod, lambda xx: _teacher_forced_next(diff, xx, mod), x0, unmask)


def test_fused_nucleus_at_72_rows():
    diff = _ar_diff(3)
    diff.config.eval.top_p = 0.8
    diff.config.eval.temperature = 0.7
    diff.config.eval.fused_nucleus = True
    B = 72
    mod = _static_mod(diff, B)
    x, nfe = diff._ar_sampler(B, modality=mod, seed=5, bos_token_id=3)
    x2, _ = diff._ar_sampler(B, modality=mod, seed=5, bos_token_id=3)
    assert nfe == 0 and torch.equal(x, x2)
    z = _teacher_forced_next(diff, x, mod)[:, :-1].masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
    probs = torch.softmax(z / 0.7, -1)
    p_tok = probs.gather(-1, x[:, 1:, None])[..., 0]
    mass_above = (probs * (probs > p_tok[..., None])).sum(-1)      # probability of the ids ranked above the drawn one
    top = probs.max(-1).values
    in_nucleus = (mass_above + p_tok <= 0.8 + 5e-2) | (p_tok >= top - 1e-4)      # (the rule and allowance of test_sampler_top_p_draws_from_the_nucleus)
    assert in_nucleus.all(), (mass_above + p_tok)[~in_nucleus]


def test_no_host_sync_and_the_cache_is_freed_at_72_rows():
    diff = _ar_diff(4)
    B, L = 72, diff.config.model.length
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
    assert nfe == L - 1 and not (x[:, 1:] == diff.mask_index).any()
    assert diff.backbone._kv is None
