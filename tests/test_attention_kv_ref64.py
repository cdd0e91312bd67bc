"""The yardstick of tests/attention_ref64.py holds at RECTANGULAR shapes (Lq queries against Lk keys, the shapes of udm_attention_fwd_kv; bidirectional, the
first Lq rows are the queries): the one-shot and the 64-key tiled bf16 emulations stay within 2u per row (O) and the lse2 bound against attention_ref64 on every
family - and the comparator rejects two seeded mutants of a rectangular kernel: a dropped last key tile and a key row >= Lk read from the cache."""
import pytest
import torch

import attention_kv_cases as C
import attention_ref64 as R


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES_CPU)
def test_emulations_stay_within_the_row_bounds_rectangular(Lq, Lk, D, family):
    B, H = 1, 2
    for prescaled in ((True, False) if (Lq, Lk) == (77, 333) else (True,)):   # (the engine's form everywhere, plain q at one shape)
        q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
        ref = R.attention_ref64(q, k, v, prescaled=prescaled)
        assert ref["o"].shape == (B, H, Lq, D) and torch.isfinite(ref["lse2"]).all()
        for name, fwd in (("oneshot", R.emulate_fwd_oneshot), ("tiled", R.emulate_fwd_tiled)):
            o, lse = fwd(q, k, v, prescaled=prescaled)
            assert torch.isfinite(o).all(), name
            worst, median, where = R.row_errors(o, ref["o"], ref["sc_o"])
            assert worst <= R.BOUNDS["o"], f"{name} o (prescaled={prescaled}): worst row {worst / R.U:.2f} u at (b, h, row) = {where}, median {median / R.U:.2f} u"
            excess, where, dead_ok = R.lse_excess(lse, ref)
            assert excess <= 1.0 and dead_ok, f"{name} lse2 (prescaled={prescaled}): {excess:.2f} x its bound at {where}"


def _rejected(o, lse, ref):
    worst, _, _ = R.row_errors(o, ref["o"], ref["sc_o"])
    excess, _, _ = R.lse_excess(lse, ref)
    return worst > R.BOUNDS["o"], excess > 1.0


@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", [(48, 560), (77, 333), (8, 72)])
def test_comparator_rejects_a_dropped_last_key_tile(Lq, Lk, D):
    q, k, v = C.make_case("gauss", 1, 2, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    cut = (Lk - 1) // 64 * 64                                         # the walk ends one tile early
    bad_o, bad_lse = _rejected(*R.emulate_fwd_tiled(q, k[:, :, :cut], v[:, :, :cut], prescaled=True), ref)
    assert bad_o and bad_lse


@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", [(48, 560), (77, 333), (129, 193), (8, 72), (128, 640)])
def test_comparator_rejects_a_key_row_past_lk(Lq, Lk, D):
    """ONE cache slot behind the Lk valid ones takes part (a tile that overhangs and is not masked): the slot holds what a cache holds there - another step's key"""
    q, k, v = C.make_case("gauss", 1, 2, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    gen = torch.Generator().manual_seed(Lk)
    stale_k = (1.2 * torch.randn(1, 2, 1, D, generator=gen)).to(R.BF16)
    stale_v = (4.0 + 1.2 * torch.randn(1, 2, 1, D, generator=gen)).to(R.BF16)
    bad_o, bad_lse = _rejected(*R.emulate_fwd_tiled(q, torch.cat([k, stale_k], 2), torch.cat([v, stale_v], 2), prescaled=True), ref)
    assert bad_o and bad_lse      # (one key in Lk moves lse2 by log2(1 + 1 / Lk): over its absolute bound at every Lk of this module)
