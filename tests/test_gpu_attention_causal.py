"""Causal attention (UDM_ATTN_CAUSAL; model.full_attention=false, models/dit.py:768 / :826 / :843 is_causal=True) of the 8-wave kernels of
csrc/attention.hip against torch fp32 autograd (sdpa(is_causal=True) on fp32 copies of the bf16 operands): head dims 32 / 64 / 128, lengths that are
and are not multiples of the 64-key / 128-query tiles, q pre-scaled or not, one shape with more blocks than CUs.  Bounds are those of the
bidirectional kernels' tests (tests/test_gpu_kernels.py): O 1e-2 and dQ / dK / dV 1.5e-2 rel-RMS, lse 2e-2 absolute (natural-log units).
Exact properties: row 0 attends to key 0 alone, keys past a query never reach it (bit for bit), and the last key's dK / dV come from the last query alone."""
import math

import pytest
import torch
import torch.nn.functional as F

from golden_utils import rel_err

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def _inputs(B, L, H, D, seed, prescaled, K):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, k, v, do = (torch.randn(B * L, H * D, device=DEV, generator=g) for _ in range(4))
    qs = K.attention_q_scale(D) if prescaled else 1.0
    return (1.5 * q * qs).to(BF16), (1.5 * k).to(BF16), v.to(BF16), do.to(BF16)


def _reference(q, k, v, do, B, L, H, D, prescaled):
    """fp32 autograd; with a pre-scaled q the scores q~ k are base-2 exponents, i.e. natural-log scores times ln 2 (and dq is wrt the stored q~)"""
    scale = math.log(2.0) if prescaled else 1.0 / math.sqrt(D)
    qh, kh, vh = (t.float().reshape(B, L, H, D).transpose(1, 2).clone().requires_grad_() for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True, scale=scale)
    o.backward(do.float().reshape(B, L, H, D).transpose(1, 2))
    s = (qh.detach() @ kh.detach().transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    flat = lambda t: t.transpose(1, 2).reshape(B * L, H * D)
    return flat(o.detach()), torch.logsumexp(s, -1), flat(qh.grad), flat(kh.grad), flat(vh.grad)


def _run(K, q, k, v, do, B, L, H, D, prescaled):
    o, lse = K.attention_fwd_generic(q, k, v, B, L, H, D, q_prescaled=prescaled, causal=True)
    dq, dk, dv = K.attention_bwd_generic(q, k, v, o, do, lse, B, L, H, D, q_prescaled=prescaled, causal=True)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


SHAPES = [(D, L) for D in (32, 64, 128) for L in (128, 384, 1280, 200, 1000)]


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("D,L", SHAPES)
def test_causal_matches_torch(K, D, L, prescaled):
    B, H = 2, 3
    q, k, v, do = _inputs(B, L, H, D, 17 * L + D, prescaled, K)
    o, lse, dq, dk, dv = _run(K, q, k, v, do, B, L, H, D, prescaled)
    o_r, lse_r, dq_r, dk_r, dv_r = _reference(q, k, v, do, B, L, H, D, prescaled)
    assert torch.isfinite(lse).all() and torch.isfinite(o.float()).all()
    assert rel_err(o.float(), o_r) < 1e-2
    assert torch.allclose(lse * math.log(2.0), lse_r, atol=2e-2, rtol=1e-3)
    assert rel_err(dq.float(), dq_r) < 1.5e-2
    assert rel_err(dk.float(), dk_r) < 1.5e-2
    assert rel_err(dv.float(), dv_r) < 1.5e-2


@pytest.mark.parametrize("B,H,L,D", [(8, 16, 1280, 128), (8, 12, 1280, 64)])   # 1280 / 1536 blocks of 128 queries: more blocks than CUs
def test_causal_many_blocks(K, B, H, L, D):
    q, k, v, do = _inputs(B, L, H, D, 5, True, K)
    o, lse, dq, dk, dv = _run(K, q, k, v, do, B, L, H, D, True)
    o_r, lse_r, dq_r, dk_r, dv_r = _reference(q, k, v, do, B, L, H, D, True)
    assert rel_err(o.float(), o_r) < 1e-2
    assert torch.allclose(lse * math.log(2.0), lse_r, atol=2e-2, rtol=1e-3)
    for got, ref in ((dq, dq_r), (dk, dk_r), (dv, dv_r)):
        assert rel_err(got.float(), ref) < 1.5e-2


@pytest.mark.parametrize("D", [32, 64, 128])
def test_causal_exact_properties(K, D):
    B, H, L = 2, 2, 384
    q, k, v, do = _inputs(B, L, H, D, 3 + D, True, K)
    o, lse, dq, dk, dv = _run(K, q, k, v, do, B, L, H, D, True)
    ov = o.view(B, L, H * D)
    # row 0 sees key 0 alone: softmax weight exactly 1, O = V[0]
    assert torch.equal(ov[:, 0], v.view(B, L, H * D)[:, 0])
    # keys / values past position p never reach rows <= p.  (p + 1 a multiple of 32: one wave holds 32 query rows, and the lazy rescale of the forward
    # is a decision of the whole wave - rows past p that share a wave with row p may move its reference exponent, which changes roundings, not values)
    for p in (31, 95, 159, 255):
        k2, v2 = k.clone().view(B, L, -1), v.clone().view(B, L, -1)
        k2[:, p + 1:] = (3 * torch.randn_like(k2[:, p + 1:].float())).to(BF16)
        v2[:, p + 1:] = (3 * torch.randn_like(v2[:, p + 1:].float())).to(BF16)
        o2, lse2 = K.attention_fwd_generic(q, k2.view(B * L, -1), v2.view(B * L, -1), B, L, H, D, q_prescaled=True, causal=True)
        assert torch.equal(o2.view(B, L, -1)[:, : p + 1], ov[:, : p + 1]), p
        assert torch.equal(lse2[:, :, : p + 1], lse[:, :, : p + 1]), p
        assert not torch.equal(o2.view(B, L, -1)[:, p + 1:], ov[:, p + 1:])
    # the last key is seen by the last query alone: its dK / dV do not move when dO of every other query row changes, and q of the rows outside the
    # last query's wave (see above: rows sharing its wave could move its reference exponent, which changes roundings of O and delta, not values)
    q3, do3 = q.clone().view(B, L, -1), do.clone().view(B, L, -1)
    q3[:, : L - 32] = (q3[:, : L - 32].float() * -0.7).to(BF16)
    do3[:, :-1] = (do3[:, :-1].float() * 1.9 + 0.3).to(BF16)
    q3, do3 = q3.view(B * L, -1), do3.view(B * L, -1)
    o3, lse3 = K.attention_fwd_generic(q3, k, v, B, L, H, D, q_prescaled=True, causal=True)
    dq3, dk3, dv3 = K.attention_bwd_generic(q3, k, v, o3, do3, lse3, B, L, H, D, q_prescaled=True, causal=True)
    last = lambda t: t.view(B, L, -1)[:, -1]
    assert torch.equal(last(o3), last(o))
    assert torch.equal(last(dk3), last(dk)) and torch.equal(last(dv3), last(dv))
    # ... and they are P[L-1, L-1] dO[L-1] / dS[L-1, L-1] q[L-1]
    _, lse_r, _, dk_r, dv_r = _reference(q, k, v, do, B, L, H, D, True)
    assert rel_err(last(dv).float(), last(dv_r)) < 1.5e-2 and rel_err(last(dk).float(), last(dk_r)) < 1.5e-2


def test_causal_abi(K):
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    B, H, L, D = 1, 2, 128, 64
    q, k, v, do = _inputs(B, L, H, D, 1, True, K)
    sid = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="CAUSAL"):
        K.attention_fwd_generic(q, k, v, B, L, H, D, sample_ids=sid, q_prescaled=True, causal=True)
    o, lse = K.attention_fwd_generic(q, k, v, B, L, H, D, q_prescaled=True, causal=True)
    with pytest.raises(RuntimeError, match="CAUSAL"):
        K.attention_bwd_generic(q, k, v, o, do, lse, B, L, H, D, sample_ids=sid, q_prescaled=True, causal=True)
    d = H * D
    o2 = torch.empty_like(q)
    lse2 = torch.empty(B, H, L, device=DEV)
    with pytest.raises(RuntimeError, match="unknown flags"):   # bits other than UDM_ATTN_Q_PRESCALED | UDM_ATTN_CAUSAL stay rejected
        _lib.call("udm_attention_fwd", _p(q), _p(k), _p(v), _p(o2), _p(lse2), _p(None), _p(None), B, H, L, D, d, d, d, d, 4 | 2, _s())
    torch.cuda.synchronize()
