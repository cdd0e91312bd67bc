"""The key-split arithmetic of udm_attention_fwd_kv_split stays inside the yardstick of tests/attention_ref64.py: per-split (m, l, O) in fp32 and the weighted
combine with one bf16 rounding (tests/attention_kv_split_ref.py) are within 2u per row (O) and the lse2 bound of attention_ref64 on every family, every head dim
and every rectangular shape, with S = 2, 3 and 8 requested - and the comparator rejects three seeded mutants of a split kernel: a dropped split, a combine
without the 2^(m_s - M) weights, a split range that is off by one tile."""
import pytest
import torch

import attention_kv_cases as C
import attention_kv_split_ref as SR
import attention_ref64 as R

SPLITS = (2, 3, 8)


def test_split_ranges_are_the_plan_s():
    assert SR.split_ranges(560, 4) == [(0, 3), (3, 5), (5, 7), (7, 9)]          # 9 tiles in 4 splits: 3, 2, 2, 2
    assert SR.split_ranges(333, 3) == [(0, 2), (2, 4), (4, 6)]
    assert SR.clamp_splits(72, 8) == 2 and SR.clamp_splits(64 * 40, 40) == 32 and SR.clamp_splits(1, 3) == 1
    for Lk in (1, 64, 65, 193, 333, 560, 640, 1280):
        for S in range(1, SR.clamp_splits(Lk, 32) + 1):
            r = SR.split_ranges(Lk, S)
            assert r[0][0] == 0 and r[-1][1] == -(-Lk // 64) and all(e > b for b, e in r) and all(r[i][1] == r[i + 1][0] for i in range(S - 1))


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES_CPU)
def test_split_emulation_stays_within_the_row_bounds(Lq, Lk, D, family):
    B, H = 1, 2
    for prescaled in ((True, False) if (Lq, Lk) == (77, 333) else (True,)):
        q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
        ref = R.attention_ref64(q, k, v, prescaled=prescaled)
        for S in SPLITS:
            o, lse = SR.emulate_fwd_tiled_split(q, k, v, prescaled=prescaled, splits=S)
            assert torch.isfinite(o).all(), S
            worst, median, where = R.row_errors(o, ref["o"], ref["sc_o"])
            assert worst <= R.BOUNDS["o"], f"S={S} o (prescaled={prescaled}): worst row {worst / R.U:.2f} u at (b, h, row) = {where}, median {median / R.U:.2f} u"
            excess, where, dead_ok = R.lse_excess(lse, ref)
            assert excess <= 1.0 and dead_ok, f"S={S} lse2 (prescaled={prescaled}): {excess:.2f} x its bound at {where}"


def test_one_split_is_the_unsplit_emulation():
    q, k, v = C.make_case("spikes", 1, 2, 77, 333, 64, prescaled=True)
    o1, l1 = SR.emulate_fwd_tiled_split(q, k, v, prescaled=True, splits=1)
    o0, l0 = R.emulate_fwd_tiled(q, k, v, prescaled=True)
    assert torch.equal(o1, o0) and torch.equal(l1, l0)


def _rejected(o, lse, ref):
    worst, _, _ = R.row_errors(o, ref["o"], ref["sc_o"])
    excess, _, _ = R.lse_excess(lse, ref)
    return worst > R.BOUNDS["o"], excess > 1.0


@pytest.mark.parametrize("mutant", ["dropped_split", "unweighted", "range_off_by_one"])
@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", [(48, 560), (77, 333)])
def test_comparator_rejects_the_split_mutants(Lq, Lk, D, S, mutant):
    q, k, v = C.make_case("gauss", 1, 2, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    good_o, good_lse = _rejected(*SR.emulate_fwd_tiled_split(q, k, v, prescaled=True, splits=S), ref)
    assert not good_o and not good_lse
    bad_o, bad_lse = _rejected(*SR.emulate_fwd_tiled_split(q, k, v, prescaled=True, splits=S, mutant=mutant), ref)
    assert bad_o and bad_lse, (bad_o, bad_lse)
