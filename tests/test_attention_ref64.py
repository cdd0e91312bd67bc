"""The bounds of tests/attention_ref64.py are reachable without the code under test: a one-shot FA2-rounding emulation and a 64-key tiled online-softmax
emulation with the kernels' 2^8 lazy-exponent rule (both in torch fp32 on the CPU) stay within 2u (O, dV), 3u (dQ, dK) and the lse2 bound on every input
family, at the smallest shape of each path of tests/test_gpu_attention_rowwise.py: plain, document mask, causal and dropout."""
import pytest
import torch

import attention_ref64 as R

# (B, H, L, D, variant): the smallest shape of the generic, document-mask, causal and dropout rows of the GPU module's table (dropout bidirectional and causal)
VARIANTS = [
    (2, 3, 100, 32, "plain"),
    (3, 2, 640, 64, "doc_contiguous"),
    (3, 2, 640, 64, "doc_padding"),
    (2, 3, 200, 32, "causal"),
    (4, 3, 200, 64, "dropout"),
    (4, 3, 200, 64, "dropout_causal"),
]
P_DROP, SEED = 0.25, 0x5EED0123456789


def _variant_kwargs(variant, B, H, L):
    kw = dict(sample_ids=None, causal=False)
    keep = None
    if variant.startswith("doc_"):
        kw["sample_ids"] = R.doc_layouts(B, L)[variant[4:]]
    if variant.endswith("causal"):
        kw["causal"] = True
    if variant.startswith("dropout"):
        keep = R.dropref.keep_mask(SEED, P_DROP, B, H, L)
    return kw, keep


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,H,L,D,variant", VARIANTS)
def test_emulations_stay_within_the_row_bounds(B, H, L, D, variant, family, prescaled):
    kw, keep = _variant_kwargs(variant, B, H, L)
    q, k, v, do = R.make_inputs(family, B, H, L, D, prescaled=prescaled, seed=L + D, **kw)
    zt = R.keep_scaled(SEED, P_DROP, B, H, L) if keep is not None else None
    ref = R.attention_ref64(q, k, v, do, prescaled=prescaled, zt=zt, **kw)
    for name, fwd in (("oneshot", R.emulate_fwd_oneshot), ("tiled", R.emulate_fwd_tiled)):
        o, lse = fwd(q, k, v, prescaled=prescaled, keep=keep, p=P_DROP, **kw)
        dq, dk, dv = R.emulate_bwd(q, k, v, o, do, lse, prescaled=prescaled, keep=keep, p=P_DROP, **kw)
        for key, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert torch.isfinite(got).all(), (name, key)
            worst, median, where = R.row_errors(got, ref[key], ref["sc_" + key])
            assert worst <= R.BOUNDS[key], f"{name} {key}: worst row {worst / R.U:.2f} u at (b, h, row) = {where}, median {median / R.U:.2f} u"
        excess, where, dead_ok = R.lse_excess(lse, ref)
        assert excess <= 1.0 and dead_ok, f"{name} lse2: {excess:.2f} x its bound at {where}"


def test_pointer_family_points():
    """query i of the pointer family puts all but ~2^-20 of its weight on key pi(i): O_i = V_pi(i) and dV_j = the sum of the dO rows that point at j"""
    B, H, L, D = 1, 2, 384, 128
    q, k, v, do = R.make_inputs("pointer", B, H, L, D, prescaled=True, seed=3)
    ref = R.attention_ref64(q, k, v, do, prescaled=True)
    s = q.double() @ k.double().transpose(-1, -2)
    pi = s.argmax(-1)
    assert all(torch.equal(pi[0, h].sort().values, torch.arange(L)) for h in range(H))      # a permutation
    o_expect = torch.gather(v.double(), 2, pi[..., None].expand(B, H, L, D))
    assert (ref["o"] - o_expect).abs().max() < 1e-4
    dv_expect = torch.zeros(B, H, L, D, dtype=torch.float64).scatter_add_(2, pi[..., None].expand(B, H, L, D), do.double())
    assert (ref["dv"] - dv_expect).abs().max() < 1e-4


def test_row_statistic_sees_one_bad_row():
    """a single row 10 % off moves the global Frobenius ratio by 3e-3 (under the 1e-2 of the global tests) and lifts the row statistic over 2u (the scale
    (P |V|) of a Gaussian row is about five times |O|, so 10 % of O is 1.8 % of the scale)"""
    B, H, L, D = 1, 1, 1000, 64
    q, k, v, _ = R.make_inputs("gauss", B, H, L, D, prescaled=True, seed=1)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    got = ref["o"].clone()
    got[0, 0, 640] *= 1.1
    worst, _, where = R.row_errors(got, ref["o"], ref["sc_o"])
    assert where == (0, 0, 640) and worst > 2 * R.BOUNDS["o"]
    assert float((got - ref["o"]).norm() / ref["o"].norm()) < 1e-2
