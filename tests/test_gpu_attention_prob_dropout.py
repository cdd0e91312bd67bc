"""Attention-probability dropout (`model.attn_dropout`) on the HIP kernels: udm_attention_fwd_dropout / udm_attention_bwd_dropout (csrc/attention.hip).

The mask the three kernels regenerate is the one include/unidisc_hip.h defines - checked exactly, through the public entry point, against the numpy
restatement of that text (tests/attn_prob_dropout_ref.py) - and forward, dQ, dK and dV agree with dense fp32 attention under the same mask to the bounds
these kernels carry against dense SDPA elsewhere (tests/test_attn_dropout.py: relative RMS 6e-3 on O, 1.5e-2 on the gradients)."""
import numpy as np
import pytest
import torch

from attn_prob_dropout_ref import dense_attention, keep_mask
from golden_utils import Golden, rel_err
from ledger import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
O_BOUND, GRAD_BOUND = 6e-3, 1.5e-2
# err(p) / err(0) per tensor: the rounding points are the same and each output sums fewer terms, so the ratio sits near 1.  Achieved, worst of the 20 cases
# (profiles/attn_prob_dropout_parity_ledger.json): O 1.065, dQ 1.047, dK 1.051, dV 1.024.  The ledger's rule (tests/ledger.py) allows up to 3 x that; 1.5 is
# asserted - a ratio above it would say the mask costs accuracy, which wants an explanation and not a wider bound.
RATIO_BOUND = dict(o=1.5, dq=1.5, dk=1.5, dv=1.5)


def _raw_fwd(q, k, v, B, L, H, D, flags, p, seed, entry="udm_attention_fwd_dropout"):
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    d = H * D
    o = torch.empty((B * L, d), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=q.device)
    tail = (float(p), int(seed)) if entry.endswith("_dropout") else ()
    _lib.call(entry, _p(q), _p(k), _p(v), _p(o), _p(lse), None, None, B, H, L, D, d, d, d, d, flags, *tail, _s())
    return o, lse


def _raw_bwd(q, k, v, o, do, lse, B, L, H, D, flags, p, seed, entry="udm_attention_bwd_dropout"):
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    d = H * D
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty((3, B, H, L), dtype=torch.float32, device=q.device)
    tail = (float(p), int(seed)) if entry.endswith("_dropout") else ()
    _lib.call(entry, _p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), None, None, B, H, L, D, d, d, d, d, d, d, d, d, flags, *tail, _s())
    return dq, dk, dv


# ------------------------------------------------------------------------------------------------ 5. the kernel's mask is the restated mask
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("D,H,L,B,causal", [(128, 16, 1280, 1, False), (128, 2, 320, 4, False), (128, 2, 320, 4, True), (64, 3, 200, 4, False),
                                            (32, 2, 130, 4, False), (32, 2, 130, 4, True)])
def test_kernel_mask_is_the_restated_mask(D, H, L, B, causal, p):
    """q = k = 0: P is uniform over the visible keys.  V = an identity block in key rows [c D, (c + 1) D) of every head, zero elsewhere: then
    O[i, h D + e] != 0 iff Z[b, h, i, c D + e] (and the key is visible).  Swept over all ceil(L / D) key blocks; no tolerance."""
    from unidisc_amd import kernels as K

    seed = 0x1234567 + 977 * L + D
    d = H * D
    keep = torch.from_numpy(keep_mask(seed, p, B, H, L))
    if causal:
        keep = keep & torch.ones(L, L, dtype=torch.bool).tril()
    z = torch.zeros(B * L, d, dtype=torch.bfloat16, device=DEV)
    got = torch.zeros(B, H, L, L, dtype=torch.bool)
    for c in range((L + D - 1) // D):
        n = min(D, L - c * D)
        v = torch.zeros(B, L, H, D, dtype=torch.bfloat16, device=DEV)
        v[:, c * D:c * D + n, :, :n] = torch.eye(n, dtype=torch.bfloat16, device=DEV)[None, :, None, :]
        o, _ = K.attention_fwd_generic(z, z, v.reshape(B * L, d), B, L, H, D, causal=causal, dropout_p=p, seed=seed)
        o = o.reshape(B, L, H, D).permute(0, 2, 1, 3).cpu()            # [B, H, i, e]
        got[:, :, :, c * D:c * D + n] = o[..., :n] != 0
        assert not bool((o[..., n:] != 0).any())
    assert torch.equal(got, keep)
    assert 0.5 * p < 1.0 - float(got.sum()) / float((torch.ones(L, L).tril() if causal else torch.ones(L, L)).sum() * B * H) < 1.5 * p


# ------------------------------------------------------------------------------------------------ 6. forward and backward against dense fp32
def _inputs(D, H, L, B, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(B * L, H * D, generator=gen) * 0.7).bfloat16() for _ in range(4))


def _dense_ref(q, k, v, do, B, L, H, D, keep, p, causal, qs=1.0):
    qq, kk, vv = (t.float().clone().requires_grad_() for t in (q, k, v))
    ref = dense_attention(qq / qs, kk, vv, B, L, H, D, keep=keep, p=p, causal=causal)
    ref.backward(do.float())
    return ref.detach(), qq.grad, kk.grad, vv.grad


CASES6 = [(128, 2, 320, 4, False, False), (128, 2, 320, 4, True, False), (128, 2, 320, 4, False, True), (128, 2, 320, 4, True, True),
          (64, 3, 200, 4, False, False), (64, 3, 200, 4, True, False), (32, 2, 130, 4, False, False), (32, 2, 130, 4, True, False),
          (128, 16, 1280, 1, False, False), (128, 16, 1280, 1, True, False)]


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("D,H,L,B,causal,prescaled", CASES6)
def test_forward_and_backward_match_dense_fp32_with_the_same_mask(D, H, L, B, causal, prescaled, p):
    from unidisc_amd import kernels as K

    seed = (1 << 40) + 31 * L + D
    q, k, v, do = _inputs(D, H, L, B)
    qs = K.attention_q_scale(D) if prescaled else 1.0
    if prescaled:
        q = (q.float() * qs).bfloat16()      # the stored, pre-scaled q (one rounding); the gradient is taken with respect to it
    keep = keep_mask(seed, p, B, H, L)
    ref = _dense_ref(q, k, v, do, B, L, H, D, keep, p, causal, qs)
    ref0 = _dense_ref(q, k, v, do, B, L, H, D, None, 0.0, causal, qs)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    kw = dict(q_prescaled=prescaled, causal=causal)
    got, got0 = [], []
    for dst, dkw in ((got, dict(dropout_p=p, seed=seed)), (got0, {})):
        o, lse = K.attention_fwd_generic(qd, kd, vd, B, L, H, D, **kw, **dkw)
        dst.extend([o] + list(K.attention_bwd_generic(qd, kd, vd, o, dod, lse, B, L, H, D, **kw, **dkw)))
    T = f"attn_prob_dropout[D{D},H{H},L{L},B{B},{'causal' if causal else 'full'}{',prescaled' if prescaled else ''},p{p}]"
    for name, g, g0, r, r0, bound in zip(("o", "dq", "dk", "dv"), got, got0, ref, ref0, (O_BOUND, GRAD_BOUND, GRAD_BOUND, GRAD_BOUND)):
        e, e0 = rel_err(g.float().cpu(), r), rel_err(g0.float().cpu(), r0)
        print(f"{T} {name}: err(p) = {e:.3e}  err(0) = {e0:.3e}  ratio = {e / e0:.3f}")
        check(T, f"{name}_relrms_vs_dense_fp32", e, bound)
        check(T, f"{name}_err_ratio_p_over_p0", e / e0, RATIO_BOUND[name])
    # and it is not the undropped result: sum_j (s Z_ij - 1) P_ij v_j has relative RMS ~ sqrt(p / (1 - p)) for zero-mean v
    dist = rel_err(got[0].float().cpu(), got0[0].float().cpu())
    print(f"{T} o: distance to the p = 0 output = {dist:.3f}")
    assert dist > 0.1


# ------------------------------------------------------------------------------------------------ 7. p = 0 is today's path; determinism
@pytest.mark.parametrize("D,H,L,B,prescaled", [(128, 16, 1280, 1, True), (64, 3, 200, 4, False)])
def test_p_zero_is_the_existing_path_bit_for_bit(D, H, L, B, prescaled):
    from unidisc_amd import kernels as K

    q, k, v, do = (t.to(DEV) for t in _inputs(D, H, L, B, seed=5))
    flags = K.ATTN_Q_PRESCALED if prescaled else 0
    o0, lse0 = _raw_fwd(q, k, v, B, L, H, D, flags, 0, 0, entry="udm_attention_fwd")
    g0 = _raw_bwd(q, k, v, o0, do, lse0, B, L, H, D, flags, 0, 0, entry="udm_attention_bwd")
    o1, lse1 = _raw_fwd(q, k, v, B, L, H, D, flags, 0.0, 99)
    g1 = _raw_bwd(q, k, v, o1, do, lse1, B, L, H, D, flags, 0.0, 99)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # the same seed twice: identical; another seed: not
    runs = []
    for seed in (7, 7, 8):
        o, lse = _raw_fwd(q, k, v, B, L, H, D, flags, 0.1, seed)
        runs.append((o, lse) + _raw_bwd(q, k, v, o, do, lse, B, L, H, D, flags, 0.1, seed))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[0][1], runs[2][1])                                          # lse is that of the undropped probabilities: no seed in it
    assert torch.allclose(runs[0][1], lse0, atol=1e-4, rtol=1e-5)                       # (lse0 may come from another kernel: the generated program)
    for i in (0, 2, 3, 4):
        assert not torch.equal(runs[0][i], runs[2][i]), i


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors():
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    lib = _lib.load()
    B, L, H, D = 2, 64, 2, 64
    d = H * D
    q, k, v, do = (t.to(DEV) for t in _inputs(D, H, L, B))
    o = torch.full((B * L, d), 7.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=DEV)
    sid = torch.zeros((B, L), dtype=torch.int64, device=DEV)
    rng = torch.zeros((B, 1, 8), dtype=torch.int32, device=DEV)
    dq, dk, dv = (torch.full_like(q, 7.0) for _ in range(3))
    delta = torch.empty((3, B, H, L), dtype=torch.float32, device=DEV)

    def fwd(p, sample_ids=None, doc_ranges=None):
        return lib.udm_attention_fwd_dropout(_p(q), _p(k), _p(v), _p(o), _p(lse), _p(sample_ids), _p(doc_ranges), B, H, L, D, d, d, d, d, 0, p, 5, _s())

    def bwd(p, sample_ids=None, doc_ranges=None):
        return lib.udm_attention_bwd_dropout(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), _p(sample_ids), _p(doc_ranges), B, H, L, D,
                                             d, d, d, d, d, d, d, d, 0, p, 5, _s())

    for call in (fwd, bwd):
        for args in ((-0.1,), (1.0,), (1.5,), (float("nan"),), (0.1, sid), (0.1, sid, rng)):
            assert call(*args) != 0, (call.__name__, args)
            msg = lib.udm_last_error().decode()
            assert "dropout" in msg and ("p_drop" in msg), msg
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and all(bool((t == 7.0).all()) for t in (dq, dk, dv))     # nothing was launched
    assert fwd(0.5) == 0 and bwd(0.5) == 0
    torch.cuda.synchronize()
    assert not bool((o == 7.0).all())


# ------------------------------------------------------------------------------------------------ 9. the model
def _model(kind, attn_dropout, ckpt=False):
    from unidisc_amd import Diffusion

    if kind == "ar":
        from ar_utils import ArGolden, ar_config

        g = ArGolden("ar_b_small")
        cfg, params = ar_config(g.case), g.params()
    else:
        from product_utils import product_config

        g = Golden("b_small")
        cfg, params = product_config(g.case), g.params()
    cfg.model.attn_dropout = attn_dropout
    diff = Diffusion(cfg, None, DEV)
    diff.backbone.load_state_dict(params, strict=True)
    diff.backbone.to(DEV)
    diff.backbone.train()
    diff.backbone.use_gradient_checkpointing = ckpt
    diff.rng_device = "cpu"
    return g, diff


def _train_step(g, diff, seed=17):
    torch.manual_seed(seed)
    out = diff.training_step(g.batch(), 1)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().clone(), {k: p.grad.clone() for k, p in diff.backbone.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["diffusion", "ar"])
def test_model_trains_with_attention_dropout(kind):
    g, diff = _model(kind, 0.1)
    assert diff.backbone.attn_dropout == pytest.approx(0.1) and diff.backbone.causal == (kind == "ar")
    loss, grads = _train_step(g, diff)
    assert torch.isfinite(loss) and grads and all(bool(torch.isfinite(t).all()) for t in grads.values())
    loss_2nd, _ = _train_step(g, diff)                      # the same data and torch seed, the next training forward: another mask
    assert not torch.equal(loss_2nd, loss)
    g, again = _model(kind, 0.1)                            # a fresh model, the same torch seed: the same mask
    loss_b, grads_b = _train_step(g, again)
    assert torch.equal(loss_b, loss)
    lin = [k for k in grads if grads[k].dim() == 2 and "embed" not in k]
    assert lin and all(torch.equal(grads[k], grads_b[k]) for k in lin)
    g, ck = _model(kind, 0.1, ckpt=True)                    # gradient checkpointing: the recompute regenerates the same masks
    loss_c, grads_c = _train_step(g, ck)
    assert torch.equal(loss_c, loss) and grads_c.keys() == grads.keys()
    for k in grads:
        # (the Linears' weight gradients are written whole by their wgrad kernels: bit for bit.  Vectors and embeddings are accumulated with fp32 atomics and
        # differ between any two runs, with or without checkpointing or dropout: the bound of tests/test_gpu_ar.py / tests/test_gpu_e2e.py for them)
        if k in lin:
            assert torch.equal(grads[k], grads_c[k]), k
        else:
            assert rel_err(grads_c[k].cpu(), grads[k].cpu()) < 2e-3, k
    g, plain = _model(kind, None)
    loss_0, _ = _train_step(g, plain)
    assert not torch.equal(loss_0, loss)                    # the mask is applied in train mode ...
    # ... and not in eval mode: the logits of the two models are the same bits
    if kind == "ar":
        x, mod = g.t("fp32/input_ids").to(DEV), g.t("fp32/modality").to(DEV)
    else:
        x, mod = g.t("fp32/xt").to(DEV), g.t("fp32/modality").to(DEV)
    sigma = torch.full((x.shape[0],), 0.5, device=DEV) if diff.backbone.time_conditioning else None
    diff.backbone.eval()
    plain.backbone.eval()
    with torch.no_grad():
        assert torch.equal(diff.backbone(x, sigma, modality=mod), plain.backbone(x, sigma, modality=mod))


# ------------------------------------------------------------------------------------------------ 10. the scale is unbiased
def test_mean_over_seeds_approaches_the_undropped_output():
    """Per seed O deviates from the p = 0 output by relative RMS sqrt(p / (1 - p)) = 0.33, independently across seeds: 0.042 expected for the mean of 64, the
    bound is 3 x that.  A scale of 1 instead of 1 / (1 - p) would leave a bias of 0.1 on top."""
    from unidisc_amd import kernels as K

    D, H, L, B, p, n = 64, 3, 200, 4, 0.1, 64
    q, k, v, _ = (t.to(DEV) for t in _inputs(D, H, L, B, seed=9))
    o0, _ = K.attention_fwd_generic(q, k, v, B, L, H, D)
    acc = torch.zeros_like(o0, dtype=torch.float32)
    for s in range(n):
        acc += K.attention_fwd_generic(q, k, v, B, L, H, D, dropout_p=p, seed=1000 + s)[0].float()
    e = rel_err((acc / n).cpu(), o0.float().cpu())
    print(f"mean over {n} seeds vs p = 0: relative RMS {e:.4f}")
    check("attn_prob_dropout[unbiased,D64,H3,L200,B4,p0.1]", "mean_of_64_seeds_relrms_vs_undropped", e, 3 * np.sqrt(p / (1 - p)) / np.sqrt(n))
