"""tests/test_attention_ref64.py at head dim 256: the two bf16 flash-attention emulations (torch fp32 on the CPU, none of the code under test) stay within the
unchanged bounds of tests/attention_ref64.py - 2u (O, dV), 3u (dQ, dK), the lse2 bound - on every input family at the shapes of
tests/test_gpu_attention_d256.py, so those bounds are reachable at D = 256."""
import pytest
import torch

import attention_ref64 as R

VARIANTS = [
    (2, 3, 100, 256, "plain"),
    (1, 3, 320, 256, "plain"),
    (3, 2, 320, 256, "doc_contiguous"),
    (3, 2, 320, 256, "doc_padding"),
    (2, 3, 200, 256, "causal"),
    (2, 3, 200, 256, "dropout"),
    (2, 3, 200, 256, "dropout_causal"),
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
def test_emulations_stay_within_the_row_bounds_d256(B, H, L, D, variant, family, prescaled):
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
