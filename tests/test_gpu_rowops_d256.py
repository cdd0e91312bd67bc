"""udm_qknorm_rope_fwd / _bwd at head dim 256: (d, D) = (512, 256), the narrow-row path, and (4096, 256), the block-per-row path of the xxl width.  Reference
(tests/fake_kernels.py), comparator and bounds are those of test_qknorm_rope in tests/test_gpu_kernels.py: 6e-3 forward, 8e-3 backward, 5e-3 on the affine
gradients."""
import pytest
import torch

import fake_kernels as R
from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels

    return kernels


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def bf(x):
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("d,D", [(512, 256), (4096, 256)])
@pytest.mark.parametrize("qk_norm", [True, False])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("q_scale", [1.0, "attention"])
def test_qknorm_rope_d256(K, d, D, qk_norm, per_sample, q_scale):
    q_scale = K.attention_q_scale(D) if q_scale == "attention" else 1.0
    B, L = 2, 20
    M = B * L
    qkv, dqkr = bf(rnd(M, 3 * d, seed=22)), bf(rnd(M, 2 * d, seed=23))
    if per_sample:
        ang = rnd(B, L, D // 2, seed=24)
    else:
        ang = rnd(L, D // 2, seed=24)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    gq, bq, gk, bk = (1 + 0.1 * rnd(d, seed=25), 0.1 * rnd(d, seed=26), 1 + 0.1 * rnd(d, seed=27), 0.1 * rnd(d, seed=28)) if qk_norm else (None,) * 4
    g = lambda t: t.to(DEV) if t is not None else None
    ref, _ = R.qknorm_rope_fwd(qkv, cos, sin, L, D, gq=gq, bq=bq, gk=gk, bk=bk, q_scale=q_scale)
    out, stats = K.qknorm_rope_fwd(g(qkv), g(cos), g(sin), L, D, gq=g(gq), bq=g(bq), gk=g(gk), bk=g(bk), q_scale=q_scale)
    assert rel_err(out.float().cpu()[:, :d], ref.float()[:, :d]) < 6e-3 and rel_err(out.float().cpu()[:, d:], ref.float()[:, d:]) < 6e-3
    dqkv_r = torch.zeros(M, 3 * d, dtype=torch.bfloat16)
    grads_r = [torch.zeros(d) for _ in range(4)] if qk_norm else [None] * 4
    R.qknorm_rope_bwd(dqkr, qkv, dqkv_r, cos, sin, L, D, gq=gq, gk=gk, dgq=grads_r[0], dbq=grads_r[1], dgk=grads_r[2], dbk=grads_r[3], q_scale=q_scale)
    dqkv = torch.zeros(M, 3 * d, dtype=torch.bfloat16, device=DEV)
    grads = [torch.zeros(d, device=DEV) for _ in range(4)] if qk_norm else [None] * 4
    K.qknorm_rope_bwd(g(dqkr), g(qkv), dqkv, g(cos), g(sin), L, D, gq=g(gq), gk=g(gk), stats=stats, dgq=grads[0], dbq=grads[1], dgk=grads[2], dbk=grads[3], q_scale=q_scale)
    assert rel_err(dqkv.float().cpu()[:, :d], dqkv_r.float()[:, :d]) < 8e-3 and rel_err(dqkv.float().cpu()[:, d:2 * d], dqkv_r.float()[:, d:2 * d]) < 8e-3
    assert torch.all(dqkv.cpu()[:, 2 * d:] == 0)
    if qk_norm:
        for a, b in zip(grads, grads_r):
            assert rel_err(a.cpu(), b) < 5e-3
