"""The three kernels of KV-cached AR decoding (csrc/decode.hip) against torch fp32: decode attention with its cache append, the skinny GEMM at the decode
shapes of UniDisc-S and the 1.4 B model with every epilogue, and the token choice (argmax of z + Gumbel with ties, restriction, guidance, x0 write-back,
Philox determinism and statistics)."""
import math

import pytest
import torch

from golden_utils import rel_err
from unidisc_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bf(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16).to(DEV)


# ------------------------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("p", [0, 63, 64, 65, 1000, 4095])
@pytest.mark.parametrize("B,H", [(3, 5), (8, 16)])
def test_attention_decode_matches_torch(D, p, B, H):
    gen = torch.Generator().manual_seed(D * 10007 + p + B)
    d, Lmax = H * D, 4096
    qs = K.attention_q_scale(D)
    q = (torch.randn(B, d, generator=gen) * qs).to(torch.bfloat16).to(DEV)
    qkr = torch.empty(B, 2 * d, dtype=torch.bfloat16, device=DEV)     # (the engine's operand layout: q | k rows of qkr, v in qkv[:, 2d:])
    qkr[:, :d] = q
    qkr[:, d:] = _bf((B, d), gen)
    qkv = _bf((B, 3 * d), gen)
    Kc, Vc = _bf((B, Lmax, d), gen), _bf((B, Lmax, d), gen)     # sentinel content everywhere: only slot p may change
    K0, V0 = Kc.clone(), Vc.clone()
    ws = K.attention_decode_ws(B, H, D, DEV)
    o = K.attention_decode(qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], Kc, Vc, p, H, D, ws=ws)
    torch.cuda.synchronize()
    keep = torch.ones(Lmax, dtype=torch.bool)
    keep[p] = False
    assert torch.equal(Kc[:, keep.to(DEV)], K0[:, keep.to(DEV)]) and torch.equal(Vc[:, keep.to(DEV)], V0[:, keep.to(DEV)])
    assert torch.equal(Kc[:, p], qkr[:, d:]) and torch.equal(Vc[:, p], qkv[:, 2 * d:])
    k = Kc[:, :p + 1].float().view(B, p + 1, H, D)
    v = Vc[:, :p + 1].float().view(B, p + 1, H, D)
    s = torch.einsum("bhd,blhd->bhl", q.float().view(B, H, D), k) * math.log(2.0)   # q holds q log2(e) / sqrt(D): base-2 scores
    ref = torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), v).reshape(B, d)
    assert rel_err(o.float(), ref) < 8e-3
    assert float((o.float() - ref).abs().max()) < 2e-2


# ------------------------------------------------------------------------------------------------ skinny GEMM
# (N, K): qkv, out-proj, MLP up, MLP down, vocabulary head - 1.4 B (d = 2048, V = 48 385) and UniDisc-S (d = 768, V = 40 193)
SHAPES = [(6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192), (48385, 2048), (2304, 768), (768, 768), (3072, 768), (768, 3072), (40193, 768)]


def _skinny_case(M, N, Kd, epi, out_f32, seed):
    gen = torch.Generator().manual_seed(seed)
    a = _bf((M, Kd), gen)
    Np = (N + 127) // 128 * 128                      # the head's weight shadow has padded rows, its logits buffer a padded row stride
    w = _bf((Np, Kd), gen, 1.0 / math.sqrt(Kd))
    bias = (torch.randn(N, generator=gen) * 0.5).to(DEV)
    out = torch.full((M, Np), float("nan"), dtype=torch.float32 if out_f32 else torch.bfloat16, device=DEV)
    K.gemm_skinny(a, w, out=out, N=N, epilogue=epi, bias=bias if epi != K.EPI_NONE else None)
    ref = a.float() @ w[:N].float().t()
    if epi != K.EPI_NONE:
        ref = ref + bias
    if epi == K.EPI_BIAS_GELU:
        ref = torch.nn.functional.gelu(ref.bfloat16().float(), approximate="tanh")
    return out, ref


@pytest.mark.parametrize("M", [1, 8, 13, 64])
@pytest.mark.parametrize("N,Kd", SHAPES)
def test_gemm_skinny_matches_torch(M, N, Kd):
    out, ref = _skinny_case(M, N, Kd, K.EPI_NONE, False, M * 7 + N + Kd)
    assert torch.isnan(out[:, N:].float()).all()        # nothing past N is written
    assert rel_err(out[:, :N].float(), ref) < 6e-3


@pytest.mark.parametrize("M", [8, 13])
@pytest.mark.parametrize("epi,out_f32", [(K.EPI_BIAS, False), (K.EPI_BIAS_GELU, False), (K.EPI_NONE, True), (K.EPI_BIAS, True)])
@pytest.mark.parametrize("N,Kd", [(8192, 2048), (2048, 8192), (48385, 2048), (3072, 768)])
def test_gemm_skinny_epilogues(M, epi, out_f32, N, Kd):
    out, ref = _skinny_case(M, N, Kd, epi, out_f32, M + N + 3 * Kd + epi)
    assert rel_err(out[:, :N].float(), ref) < (1e-4 if out_f32 else 6e-3)


def test_gemm_skinny_small_model_shapes():
    """the test models' decode shapes (d = 64: K = 64 / 256, N below one 32-column tile)"""
    for N, Kd in ((192, 64), (64, 64), (256, 64), (64, 256), (65, 64)):
        out, ref = _skinny_case(8, N, Kd, K.EPI_BIAS, False, N + Kd)
        assert rel_err(out[:, :N].float(), ref) < 6e-3


# ------------------------------------------------------------------------------------------------ token choice
def _rows(R, V, gen, ld=None, quantise=False):
    ld = ld or (V + 7) // 8 * 8
    lg = torch.randn(R, ld, generator=gen) * 3
    if quantise:   # few distinct values: many exact ties
        lg = lg.round()
    return lg.to(torch.bfloat16).to(DEV)


def _excluded(R, V, Vt, mask_id, nxt_mod):
    ids = torch.arange(V, device=DEV)
    bad = (ids == mask_id)[None].expand(R, V)
    if nxt_mod is not None:
        bad = bad | torch.where((nxt_mod == 1)[:, None], ids[None] < Vt, ids[None] >= Vt)
    return bad


@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("restrict", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_ar_sample_rows_explicit_noise(quantise, restrict, guided):
    gen = torch.Generator().manual_seed(int(quantise) + 2 * int(restrict) + 4 * int(guided))
    R, V, Vt, mask_id, L, pos = 6, 1000, 700, 699, 12, 5
    logits = _rows(2 * R if guided else R, V, gen, quantise=quantise)
    w = torch.full((4,), 1.5, device=DEV)
    g = torch.zeros(R, 3 * V + 8, device=DEV) if quantise else torch.randn(R, 3 * V + 8, generator=gen).to(DEV)
    modality = torch.randint(0, 2, (R, L), generator=gen).to(DEV)
    x0 = torch.randint(0, V, (R, L), generator=gen).to(DEV)
    unmask = torch.zeros(R, L, dtype=torch.bool, device=DEV)
    unmask[1, pos] = unmask[4, pos] = True
    x = torch.full((R, L), -5, dtype=torch.int64, device=DEV)
    nxt = torch.full((2 * R,), -9, dtype=torch.int64, device=DEV)
    K.ar_sample_rows(logits, x, pos, V, Vt, mask_id, step=3, modality=modality, restrict=restrict, g=g, g_col0=V + 8, x0=x0, x0_unmask=unmask, next_ids=nxt,
                     logits_u=logits[R:] if guided else None, w=w if guided else None, rows=R)
    z = logits[:R, :V].float()
    if guided:
        z = 2.5 * z - 1.5 * logits[R:, :V].float()
    z = (z + g[:, V + 8:2 * V + 8]).masked_fill(_excluded(R, V, Vt, mask_id, modality[:, pos] if restrict else None), float("-inf"))
    y = torch.where(unmask[:, pos], x0[:, pos], z.argmax(-1))
    assert torch.equal(x[:, pos], y)
    other = torch.ones(L, dtype=torch.bool, device=DEV)
    other[pos] = False
    assert (x[:, other] == -5).all()
    assert torch.equal(nxt[:R], y)
    if guided:
        assert torch.equal(nxt[R:], torch.where(unmask[:, pos], torch.full_like(y, mask_id), y))
    else:
        assert (nxt[R:] == -9).all()


def test_ar_sample_rows_philox_deterministic_and_gumbel():
    """Philox Gumbel: the same (seed, step) draws the same tokens, another step others; over 10^5 draws of one logit row (rows x steps, each its own noise)
    the frequencies follow softmax(logits) within a loose chi-square bound."""
    gen = torch.Generator().manual_seed(5)
    V = 16
    R, steps = 1000, 100
    row = (torch.randn(V, generator=gen)).to(torch.bfloat16)
    logits = torch.zeros(R, 16, dtype=torch.bfloat16)
    logits[:, :V] = row
    logits = logits.to(DEV)
    x = torch.zeros(R, 2, dtype=torch.int64, device=DEV)
    counts = torch.zeros(V, dtype=torch.float64)
    first = None
    for s in range(steps):
        K.ar_sample_rows(logits, x, 1, V, 0, V + 100, step=s, seed=1234)   # (mask id outside the row: nothing excluded)
        counts += torch.bincount(x[:, 1].cpu(), minlength=V).double()
        if s == 0:
            first = x[:, 1].clone()
    x2 = torch.zeros_like(x)
    K.ar_sample_rows(logits, x2, 1, V, 0, V + 100, step=0, seed=1234)
    assert torch.equal(x2[:, 1], first)
    K.ar_sample_rows(logits, x2, 1, V, 0, V + 100, step=1, seed=1234)
    assert not torch.equal(x2[:, 1], first)
    n = R * steps
    expect = torch.softmax(row.float().double(), 0) * n
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 60.0, (chi2, counts, expect)   # 15 degrees of freedom: p(chi2 > 60) ~ 1e-7
