"""CPU checks of tests/nucleus_ref64.py, the fp64 reference the fused top-p kernels are held to on the GPU (tests/test_gpu_nucleus_rows.py):
two independent fp32 emulations stay inside delta on every input family, the comparator rejects every seeded mutant, the reference's own
`nucleus_sampling_batch` / `nucleus_sampling` formulas give kept sets the comparator accepts, the fp64 race leaves at most 1 % of the GPU test's rows
undecided, and torch's multinomial path passes the chi-square statistic the Philox draws are held to."""
import pytest
import torch

import nucleus_ref64 as N

F32 = torch.float32
SMALL = [(64, 43, 40, 24), (1000, 611, 600, 6)]          # (V, Vt, mask_id, M)


def _ref(c, rule):
    inv_t, budget = N.RULES[rule]
    return N.Ref(c["zc"], c["zu"], c["w"], c["valid"], inv_t, budget, c["V"])


@pytest.mark.parametrize("rule", sorted(N.RULES))
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("V,Vt,mask_id,M", SMALL)
def test_fp32_emulations_stay_inside_delta(V, Vt, mask_id, M, guided, rule):
    inv_t, budget = N.RULES[rule]
    for family in N.FAMILIES:
        for restrict in (False, True):
            c = N.case(family, V, Vt, mask_id, M, restrict=restrict, guided=guided)
            ref = _ref(c, rule)
            exact, tok = N.emulate(c["zc"], c["zu"], c["w"], c["valid"], inv_t, budget, c["u"], V)
            assert torch.equal(exact, ref.n) and ref.judge(exact, tok, c["u"]) == [], (family, restrict)
            for arith in ("seq32", "hist32"):
                keep, _ = N.emulate(c["zc"], c["zu"], c["w"], c["valid"], inv_t, budget, c["u"], V, arith=arith)
                acc = ref.accepts(keep)
                assert bool(acc.all()), (family, restrict, arith, keep[~acc].tolist(), ref.n[~acc].tolist())


def test_families_hold_what_they_promise():
    V, Vt, mask_id, M = 1000, 611, 600, 6
    b = N.RULES["batch"][1]
    ref = lambda f, **kw: _ref(N.case(f, V, Vt, mask_id, M, restrict=True, guided=False, **kw), "batch")
    r = ref("peak")
    assert r.n.tolist() == [1, 1, 2, 1, 1, 2]                       # one peak, two tied (0.5 each: the second does not fit), three tied (two fit)
    c = N.case("peak", V, Vt, mask_id, M, restrict=True, guided=False)
    tied = (c["zc"][1, :V].float() == 40.0).nonzero()[:, 0]
    assert int(r.order[1, 0]) == int(tied.min())                    # first index on a tied peak
    r = ref("flat")
    fl, clear = N.flat_floor(r)
    assert bool(clear.all()) and torch.equal(r.n, fl)               # the floor is not in doubt at these sizes
    c = N.case("flat", V, Vt, mask_id, M, restrict=True, guided=False)
    for row in range(M):
        assert torch.equal(r.order[row, : int(r.n[row])], c["valid"][row].nonzero()[:, 0][: int(r.n[row])])      # exactly the first floor-many ids
    r, c = ref("plateaus"), N.case("plateaus", V, Vt, mask_id, M, restrict=True, guided=False)
    for row in range(M):
        n1 = int((c["zc"][row, :V].float() == 2.0).sum())
        n2 = int(((c["zc"][row, :V].float() == 0.0) & c["valid"][row]).sum())
        assert n1 < int(r.n[row]) < n1 + n2                          # the cut lies inside the second plateau
    assert ref("neg300").n.tolist() == [1] * M
    r, c = ref("spikes"), N.case("spikes", V, Vt, mask_id, M, restrict=True, guided=False)
    assert bool(c["valid"].gather(1, r.order[:, :1]).all())


def test_comparator_rejects_every_mutant():
    V, Vt, mask_id, M = 1000, 611, 600, 6
    for name in N.MUTANTS:
        caught = []
        for family in N.FAMILIES:
            c = N.case(family, V, Vt, mask_id, M, restrict=True, guided=False)
            keep, tok = N.run_mutant(name, c)
            if _ref(c, "batch").judge(keep, tok, c["u"]):
                caught.append(family)
        assert caught, f"mutant {name} passes the comparator on every family"


def _nucleus_sampling_batch_kept(p, top_p, temperature):
    """model_eval.py:2642-2685 restated: kept count per row (sort, cumsum of p / temperature <= top_p, the top id forced)"""
    sp = torch.sort(p / temperature, descending=True, dim=-1)[0]
    keep = sp.cumsum(-1) <= top_p
    keep[..., 0] = True
    return keep.sum(-1)


def _nucleus_sampling_kept(z, top_p, temperature):
    """model_eval.py:2691-2734 restated, as in tests/test_ar_sampler_host.py"""
    sp = torch.sort(torch.softmax(z / temperature, dim=-1), descending=True, dim=-1)[0]
    mask = torch.cumsum(sp, dim=-1) <= top_p
    mask[..., 0] = True
    return mask.sum(-1)


@pytest.mark.parametrize("family", N.FAMILIES)
def test_reference_formulas_are_this_rule(family):
    V, Vt, mask_id, M = 1000, 611, 600, 6
    c = N.case(family, V, Vt, mask_id, M, restrict=True, guided=False)
    z = c["zc"][:, :V].float().masked_fill(~c["valid"], float("-inf"))
    kb = _nucleus_sampling_batch_kept(torch.softmax(z, -1), N.TOP_P, N.TEMPERATURE)
    acc = _ref(c, "batch").accepts(kb)
    assert bool(acc.all()), (kb.tolist(), _ref(c, "batch").n.tolist())
    ka = _nucleus_sampling_kept(z, N.TOP_P, N.TEMPERATURE)
    acc = _ref(c, "ar").accepts(ka)
    assert bool(acc.all()), (ka.tolist(), _ref(c, "ar").n.tolist())


@pytest.mark.parametrize("V,Vt,mask_id,M,restrict,guided", N.GPU_CASES)
def test_fp64_race_decides_the_gpu_cases(V, Vt, mask_id, M, restrict, guided):
    for rule in sorted(N.RULES):
        for family in N.FAMILIES:
            c = N.case(family, V, Vt, mask_id, M, restrict=restrict, guided=guided)
            ref = _ref(c, rule)
            _, decided = ref.race(ref.n, c["u"])
            assert int((~decided).sum()) * 100 <= M, (family, rule)


def test_multinomial_path_passes_the_chi_square_statistic():
    """the tensor path's draw (multinomial of the renormalised kept probabilities) under the statistic the Philox draws of the kernel are held to"""
    inv_t, budget = N.RULES["batch"]
    for i, row in enumerate(N.chi_rows()):
        zc = row[None]
        valid = torch.ones(1, N.CHI_V, dtype=torch.bool)
        ref = N.Ref(zc, None, None, valid, inv_t, budget, N.CHI_V)
        n = int(ref.n[0])
        kept = ref.order[0, :n]
        expect = ref.p[0, kept] / ref.S[0, n - 1]
        assert n >= 4 and float(expect.min()) > 2e-3
        fp = torch.zeros(N.CHI_V, dtype=F32)
        fp[kept] = expect.float()
        tok = torch.multinomial(fp.expand(N.CHI_ROWS, -1), 1, generator=torch.Generator().manual_seed(11 + i))[:, 0]
        stat, outside = N.pearson(tok, expect, kept)
        assert outside == 0 and stat < N.chi2_quantile(n - 1), (i, stat, N.chi2_quantile(n - 1))
    assert abs(N.chi2_quantile(10) - 52.0) < 6.0        # chi-square(10) at 1 - 1e-6 is 46.9 ... Wilson-Hilferty at z = 4.75 lands next to it
