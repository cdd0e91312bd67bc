"""The yardstick of tests/attention_ref64.py holds under the RECTANGULAR CAUSAL mask (udm_attention_fwd_kv_causal: query i of Lq sees the keys
j <= i + (Lk - Lq)): the one-shot and the 64-key tiled bf16 emulations stay within the bounds of tests/test_gpu_attention_kv_causal_rowwise.py - 2u per row
for O, the fp32 dot-product bound for lse2 - against attention_ref64(causal=True) on every case, and the comparator rejects four mutants of the mask:
    strict        j <  i + off              (the diagonal is lost)
    no_offset     j <= i                    (the mask of the square call)
    one_more      j <= i + off + 1          (one key too many)
    tile_rounded  j <  64 ceil((i + off + 1) / 64), j < Lk   (the frontier rounded up to its key tile: a tile walk without the per-element test)
Each must fail the O or the lse2 bound in every family at the shapes with Lq > 1 and Lk > Lq (at Lq = Lk `no_offset` IS the mask, at Lq = 1 the last two
cannot show).  Some show through lse2 alone (the strict diagonal on `pointer` at (77, 333): O 0.9 u, lse2 23 x its bound), so both bounds are the check."""
import pytest
import torch

import attention_kv_causal_cases as C
import attention_ref64 as R


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES)
def test_emulations_stay_within_the_row_bounds_causal(Lq, Lk, D, family):
    B, H = 1, 2
    for prescaled in ((True, False) if (Lq, Lk) == (77, 333) else (True,)):   # (the engine's form everywhere, plain q at one shape)
        q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
        ref = R.attention_ref64(q, k, v, prescaled=prescaled, causal=True)
        assert ref["o"].shape == (B, H, Lq, D) and torch.isfinite(ref["lse2"]).all()      # key 0 is visible to every query: no dead row
        for name, fwd in (("oneshot", R.emulate_fwd_oneshot), ("tiled", R.emulate_fwd_tiled)):
            o, lse = fwd(q, k, v, prescaled=prescaled, causal=True)
            assert torch.isfinite(o).all(), name
            worst, median, where = R.row_errors(o, ref["o"], ref["sc_o"])
            assert worst <= R.BOUNDS["o"], f"{name} o (prescaled={prescaled}): worst row {worst / R.U:.2f} u at (b, h, row) = {where}, median {median / R.U:.2f} u"
            excess, where, dead_ok = R.lse_excess(lse, ref)
            assert excess <= 1.0 and dead_ok, f"{name} lse2 (prescaled={prescaled}): {excess:.2f} x its bound at {where}"


def test_the_reference_mask_is_the_rectangular_one():
    ok = R.visible(1, 3, 5, causal=True)[0, 0]
    assert ok.tolist() == [[True, True, True, False, False], [True, True, True, True, False], [True, True, True, True, True]]


def _mask(kind, Lq, Lk):
    i, j, off = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :], Lk - Lq
    if kind == "exact":
        return j <= i + off
    if kind == "strict":
        return j < i + off
    if kind == "no_offset":
        return j <= i
    if kind == "one_more":
        return j <= i + off + 1
    if kind == "tile_rounded":
        return j < (i + off + 64) // 64 * 64
    raise ValueError(kind)


def _oneshot_masked(q, k, v, ok):
    """R.emulate_fwd_oneshot (pre-scaled q) under an arbitrary [Lq, Lk] mask in which every row sees a key"""
    s = (q.float() @ k.float().transpose(-1, -2)).masked_fill(~ok, float("-inf"))
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))
    return R._bf(R._bf(torch.exp2(s - lse)) @ v.float()), lse.squeeze(-1)


MUTANTS = ("strict", "no_offset", "one_more", "tile_rounded")


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.MUTANT_SHAPES)
def test_comparator_rejects_the_mask_mutants(Lq, Lk, D, family):
    q, k, v = C.make_case(family, 1, 2, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True, causal=True)
    o, lse = _oneshot_masked(q, k, v, _mask("exact", Lq, Lk))                # the emulation itself: the exact mask gives R.emulate_fwd_oneshot's bits
    o_r, lse_r = R.emulate_fwd_oneshot(q, k, v, prescaled=True, causal=True)
    assert torch.equal(o, o_r) and torch.equal(lse, lse_r)
    missed = []
    for kind in MUTANTS:
        o, lse = _oneshot_masked(q, k, v, _mask(kind, Lq, Lk))
        worst, _, _ = R.row_errors(o, ref["o"], ref["sc_o"])
        excess, _, _ = R.lse_excess(lse, ref)
        if not (worst > R.BOUNDS["o"] or excess > 1.0):
            missed.append(f"{kind}: O {worst / R.U:.2f} u, lse2 {excess:.2f} x its bound")
    assert not missed, "; ".join(missed)
