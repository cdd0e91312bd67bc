"""The reference, the bounds and the input families of tests/rowops_ref64.py, checked on the CPU without the code under test:

  - the preconditions of the reference (exact `ints` sums, the layout and the keep rate of the CPU Philox mask);
  - two fp32 emulations per operation that differ in reduction order (and in the last bits of rsqrt / exp) stay inside every bound on every family and width;
  - FACTOR and CE_C are what the rule of the module docstring gives for the ratios measured here at factor 1 (recorded through tests/ledger.py);
  - on every row the fp32 part of a bf16 output's bound is at most a quarter of its bf16 part;
  - the comparator rejects every seeded mutant of MUTANTS on the family built for it.
"""
import numpy as np
import pytest
import torch

import ledger
import rowops_ref64 as R

B, L = 2, 7          # two batch elements (a batch seam), 14 rows: zero rows, odd rows, a ragged wave group
TEST = "test_rowops_ref64"


def _emu(ar, **kw):
    return R.Arith(ar.dtype, ar.order, ar.rsqrt_ulps, **kw)


def _all_cases(family, d):
    """(name, case, forward, backward) of every operation at width d"""
    for nt in (0, 1):
        for mode in R.NORM_MODES:
            yield f"norm[{'rms' if nt == 0 else 'ln'},{mode}]", R.norm_case(family, B, L, d, nt, mode), R.norm_case_fwd, R.norm_case_bwd
    for variant in R.RESID_VARIANTS:
        yield f"residual[{variant}]", R.resid_case(family, B, L, d, variant), R.resid_case_fwd, R.resid_case_bwd
    for D in R.qk_heads(d)[:1] + R.qk_heads(d)[-1:]:
        for qk_norm, per_sample, qs in ((True, False, 0.18), (True, True, 1.0), (False, False, 0.18)):
            yield f"qk[D{D},norm{int(qk_norm)},ps{int(per_sample)}]", R.qk_case(family, B, L, d, D, qk_norm, per_sample, qs), R.qk_case_fwd, R.qk_case_bwd


def _worst(got, ref, fp32_part_only=False):
    """{key: worst ratio}; fp32_part_only: against E alone (the emulation then keeps its outputs unrounded)"""
    res = {}
    for k in ref:
        if k.startswith("E_") or k not in got or k.endswith("_nr"):
            continue
        res[k] = R.worst(got[k], ref[k], ref["E_" + k], (k in R.BF16_OUT) and not fp32_part_only)[0]
    for k in ("x_out", "qkr"):        # the statement without the internal rounding: u times the scaled magnitude on every element
        if k + "_nr" in ref and k in got:
            res[k + "_nr"] = R.worst(got[k], ref[k + "_nr"], ref["E_" + k + "_nr"], k in R.BF16_OUT and not fp32_part_only)[0]
    return res


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulations_stay_within_every_bound(family, d):
    worst = {}
    for name, c, fwd, bwd in _all_cases(family, d):
        ref_f = fwd(R.REF, c)
        ref_b = bwd(R.REF, c, ref_f)
        for ename, ar in R.EMULATIONS.items():
            got = dict(fwd(ar, c), **bwd(ar, c, ref_f))
            for k, r in _worst(got, dict(ref_f, **ref_b)).items():
                assert r <= 1.0, f"{name} {ename} {k}: {r:.3f} x its bound ({family}, d = {d})"
                worst[k] = max(worst.get(k, 0.0), r)
    for k, r in worst.items():
        ledger.check(TEST, f"emulation/{family}/d{d}/{k}", r, 1.0)


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_fp32_part_is_at_most_a_quarter_of_the_bf16_part(family, d):
    """the bound of a bf16 output never exceeds 1.25 x the rounding it is about"""
    worst = 0.0
    for name, c, fwd, bwd in _all_cases(family, d):
        ref = fwd(R.REF, c, flips=False)
        ref.update(bwd(R.REF, c, ref))
        for k in ("y", "h", "dbranch", "qkr", "dqk"):
            if k in ref:
                s = R.quarter_share(ref[k], ref["E_" + k])
                assert s <= 0.25, f"{name} {k}: the fp32 part is {s:.3f} of the bf16 part on some row ({family}, d = {d})"
                worst = max(worst, s)
    ledger.check(TEST, f"quarter_share/{family}/d{d}", worst, 0.25)


@pytest.mark.parametrize("d", [64, 768, 2048, 4096])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_fused_backward_emulations_stay_within_every_bound(family, d):
    """norm backward -> residual-branch backward at the updated dx (udm_norm_residual_bwd, udm_norm_residual_bwd_ada): the dx error is carried into the second half"""
    worst = {}
    for mode, variant in [("plain", v) for v in R.FUSED_VARIANTS] + list(R.FUSED_ADA_VARIANTS.values()):
        c = R.fused_case(family, B, L, d, mode, variant)
        stats = R.fused_stats(R.REF, c)
        ref = R.fused_case_bwd(R.REF, c, stats)
        assert R.quarter_share(ref["dbranch"], ref["E_dbranch"]) <= 0.25
        for ename, ar in R.EMULATIONS.items():
            for k, (r, _) in R.compare(R.fused_case_bwd(ar, c, stats), ref).items():
                assert r <= 1.0, f"fused[{mode},{variant}] {ename} {k}: {r:.3f} x its bound ({family}, d = {d})"
                worst[k] = max(worst.get(k, 0.0), r)
    for k, r in worst.items():
        ledger.check(TEST, f"emulation_fused/{family}/d{d}/{k}", r, 1.0)


def test_factor_is_the_rule_applied_to_the_measured_ratios():
    """at factor 1, with unrounded outputs: worst ratio of any emulation against the fp32 part alone; FACTOR = the smallest power of two >= 4 x that ratio"""
    worst, where = 0.0, None
    for family in R.FAMILIES:
        for d in (64, 768, 1032, 4096):
            for name, c, fwd, bwd in _all_cases(family, d):
                ref = fwd(R.REF, c, factor=1)
                ref.update(bwd(R.REF, c, ref, factor=1))
                for ename, ar in R.EMULATIONS.items():
                    ar = _emu(ar, round_out=False)
                    got = dict(fwd(ar, c), **bwd(ar, c, ref))
                    for k, r in _worst(got, ref, fp32_part_only=True).items():
                        if r > worst:
                            worst, where = r, (name, ename, k, family, d)
    print(f"worst fp32-part ratio at factor 1: {worst:.3f} at {where}")
    ledger.record(TEST, "factor1_worst_ratio", worst, note=str(where))
    ledger.record(TEST, "FACTOR", R.FACTOR)
    factor = 1
    while factor < 4 * worst:
        factor *= 2
    assert factor == R.FACTOR, (worst, where)


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("d", R.WIDTHS)
def test_ints_family_sums_are_exact(d):
    x = R.make_rows("ints", 37, d, 5)
    assert R.ints_sums_exact(x) and R.ints_sums_exact(x.to(R.BF16).float())
    for order in ("torch", "lanes"):                      # ... so two fp32 orders agree to the bit, for x and for x^2
        ar = R.Arith(R.F32, order)
        assert torch.equal(ar.rowsum(x).double(), x.double().sum(-1)) and torch.equal(ar.rowsum(x * x).double(), (x.double() ** 2).sum(-1))
    assert not R.ints_sums_exact(R.make_rows("gauss", 4, d, 5))


def test_dropout_mask_layout_and_rate():
    """element e = row d + col: field e & 7 (x.lo x.hi y.lo y.hi z.lo z.hi w.lo w.hi) of philox4x32(seed, e >> 3), kept when field >= thr"""
    M, d, p = 6, 72, 0.1
    keep = R.dropout_keep(R.SEED, p, M, d)
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    assert thr == 6554
    for e in (0, 1, 7, 8, 71, 72, 73, M * d - 1):
        w = R.dropref.philox4x32(R.SEED, np.array([e >> 3], dtype=np.uint64))
        word, half = int(w[(e & 7) >> 1][0]), (e & 7) & 1
        field = (word >> 16) if half else (word & 0xFFFF)
        assert bool(keep[e // d, e % d]) == (field >= thr), e
    big = R.dropout_keep(R.SEED, p, 256, 2048)
    n = big.numel()
    rate = float(big.double().mean())
    assert abs(rate - (1 - thr / 65536)) < 4 * (p * (1 - p) / n) ** 0.5
    assert not torch.equal(R.dropout_keep(R.SEED + 1, p, M, d), keep)
    assert R.dropout_keep(R.SEED, 0.0, M, d).all()


# ------------------------------------------------------------------------------------------------ mutants
def _rejected(got, ref, keys):
    w = _worst(got, ref)
    return max(w[k] for k in keys), w


def _norm_mutant(mutant, family, d, nt, mode, keys, bwd=False, Bm=B, Lm=L):
    c = R.norm_case(family, Bm, Lm, d, nt, mode)
    ref = R.norm_case_fwd(R.REF, c)
    ar, good = R.Arith(R.F32, "torch", mutant=mutant), R.Arith(R.F32, "torch")
    if bwd:
        refb = R.norm_case_bwd(R.REF, c, ref)
        return _rejected(R.norm_case_bwd(ar, c, ref), refb, keys)[0], _rejected(R.norm_case_bwd(good, c, ref), refb, keys)[0]
    return _rejected(R.norm_case_fwd(ar, c), ref, keys)[0], _rejected(R.norm_case_fwd(good, c), ref, keys)[0]


NORM_MUTANTS = [
    ("drop_last8", "spike_edges", 1032, 0, "plain", ("rstd", "y"), False),
    ("drop_last8", "ints", 4096, 0, "plain", ("rstd",), False),
    ("drop_last8", "gauss", 768, 1, "plain", ("dx",), True),
    ("mean_dm8", "gauss", 4096, 1, "plain", ("mean", "rstd"), False),
    ("mean_dm8", "ints", 4096, 0, "plain", ("rstd",), False),
    ("mean_dm8", "gauss", 4096, 0, "plain", ("dx",), True),
    ("onepass_var", "offset", 768, 1, "plain", ("rstd",), False),
    ("onepass_var", "offset_rows", 4096, 1, "plain", ("rstd",), False),
    ("no_eps", "tiny", 768, 0, "plain", ("rstd", "y"), False),
    ("no_eps", "zero_rows", 768, 0, "plain", ("rstd", "y"), False),
    ("no_eps", "zero_rows", 64, 1, "mod_all", ("y",), False),
    ("mod_text", "gauss", 64, 0, "mod_img", ("y",), False),
    ("mod_text", "gauss", 64, 1, "mod_img", ("dx", "dshift", "dscale"), True),
    ("batch_seam", "gauss", 64, 0, "mod_all", ("y",), False),
    ("batch_seam", "gauss", 64, 0, "mod_all", ("dx", "dshift"), True),
]


@pytest.mark.parametrize("mutant,family,d,nt,mode,keys,bwd", NORM_MUTANTS, ids=[f"{m[0]}-{m[1]}-d{m[2]}-{'ln' if m[3] else 'rms'}-{'bwd' if m[6] else 'fwd'}" for m in NORM_MUTANTS])
def test_norm_mutants_are_rejected(mutant, family, d, nt, mode, keys, bwd):
    bad, good = _norm_mutant(mutant, family, d, nt, mode, keys, bwd)
    assert good <= 1.0 and bad > 1.0, (bad, good)
    ledger.record(TEST, f"mutant/{mutant}/{family}/d{d}/{'bwd' if bwd else 'fwd'}", bad, 1.0, note="must exceed 1")


@pytest.mark.parametrize("family", ["gauss", "offset", "spike_edges"])
def test_a_single_wrong_element_is_seen(family):
    """what the Frobenius ratio of the older tests hides: one element of one row of an fp32 output off by 5e-4 relative (a dropped element of a wave sum)"""
    c = R.norm_case(family, 8, 15, 1032, 0, "plain")
    ref = R.norm_case_fwd(R.REF, c)
    got = R.norm_case_fwd(R.EMULATIONS["torch_order"], c)
    assert _worst(got, ref)["rstd"] <= 1.0
    got["rstd"] = got["rstd"].clone()
    got["rstd"][77] *= 1 + 5e-4
    assert float(((got["rstd"].double() - ref["rstd"]).norm() / ref["rstd"].norm())) < 1e-4          # invisible to a whole-tensor ratio at 1e-4
    assert _worst(got, ref)["rstd"] > 10


def test_residual_mutants_are_rejected():
    d = 768
    for mutant, variant, keys, bwd in (("dropout_ctr", "dropout", ("x_out",), False), ("dropout_ctr", "gate_sandwich_dropout", ("dbranch", "dw_b", "dgate"), True),
                                       ("batch_seam", "gate_all", ("x_out", "h"), False), ("batch_seam", "gate_all", ("dbranch", "dgate"), True),
                                       ("drop_last8", "sandwich_rms", ("rstd_b", "x_out", "rstd_n", "h"), False), ("mean_dm8", "sandwich_ln", ("mean_b", "x_out"), False),
                                       ("no_eps", "sandwich_rms", ("x_out",), False), ("mod_text", "sandwich_rms", ("h",), False)):
        family = "zero_rows" if mutant == "no_eps" else ("spike_edges" if mutant == "drop_last8" else "gauss")
        c = R.resid_case(family, B, L, d, variant)
        ref = R.resid_case_fwd(R.REF, c)
        ar, good = R.Arith(R.F32, "torch", mutant=mutant), R.Arith(R.F32, "torch")
        if bwd:
            refb = R.resid_case_bwd(R.REF, c, ref)
            bad_r, ok_r = _rejected(R.resid_case_bwd(ar, c, ref), refb, keys)[0], _rejected(R.resid_case_bwd(good, c, ref), refb, keys)[0]
        else:
            bad_r, ok_r = _rejected(R.resid_case_fwd(ar, c), ref, keys)[0], _rejected(R.resid_case_fwd(good, c), ref, keys)[0]
        assert ok_r <= 1.0 and bad_r > 1.0, (mutant, variant, bad_r, ok_r)
        ledger.record(TEST, f"mutant/{mutant}/residual[{variant}]/{'bwd' if bwd else 'fwd'}", bad_r, 1.0, note="must exceed 1")
    # the dropout mutant changes the zero pattern itself
    c = R.resid_case("gauss", B, L, d, "dropout")
    c.x_in = torch.zeros_like(c.x_in)
    a = R.resid_case_fwd(R.Arith(R.F32, "torch"), c)["x_out"]
    b = R.resid_case_fwd(R.Arith(R.F32, "torch", mutant="dropout_ctr"), c)["x_out"]
    assert torch.equal(a == 0, ~R.dropout_keep(R.SEED, c.p, c.M, d)) and not torch.equal(a == 0, b == 0)


def test_qk_mutants_are_rejected():
    d, D = 768, 64
    for mutant, keys, bwd, per_sample in (("rope_row", ("qkr",), False, False), ("rope_row", ("dqk",), True, False), ("rot_sign", ("qkr",), False, False),
                                          ("rot_sign", ("dqk", "dgq"), True, True), ("qscale_on_k", ("qkr",), False, False), ("qscale_on_k", ("dqk", "dgk"), True, False),
                                          ("drop_last8", ("stats", "qkr"), False, False), ("mean_dm8", ("stats",), False, True)):
        c = R.qk_case("spike_edges" if mutant == "drop_last8" else "gauss", B, L, d, D, True, per_sample, 0.18)
        ref = R.qk_case_fwd(R.REF, c)
        ar, good = R.Arith(R.F32, "torch", mutant=mutant), R.Arith(R.F32, "torch")
        if bwd:
            refb = R.qk_case_bwd(R.REF, c, ref)
            bad_r, ok_r = _rejected(R.qk_case_bwd(ar, c, ref), refb, keys)[0], _rejected(R.qk_case_bwd(good, c, ref), refb, keys)[0]
        else:
            bad_r, ok_r = _rejected(R.qk_case_fwd(ar, c), ref, keys)[0], _rejected(R.qk_case_fwd(good, c), ref, keys)[0]
        assert ok_r <= 1.0 and bad_r > 1.0, (mutant, keys, bad_r, ok_r)
        ledger.record(TEST, f"mutant/{mutant}/qk/{'bwd' if bwd else 'fwd'}", bad_r, 1.0, note="must exceed 1")


def test_assignment_instead_of_accumulation_is_rejected():
    """the accumulated outputs start from a nonzero tensor and the reference adds to it: a kernel that writes `=` is off by that tensor"""
    ar = R.Arith(R.F32, "torch")
    c = R.norm_case("gauss", B, L, 64, 0, "mod_all")
    ref = R.norm_case_fwd(R.REF, c)
    refb = R.norm_case_bwd(R.REF, c, ref)
    got = R.norm_case_bwd(ar, c, ref, prefill=False, accumulate=False)
    w = _worst(got, refb)
    assert all(w[k] > 1.0 for k in ("dx", "dw", "dshift", "dscale")), w
    c = R.resid_case("gauss", B, L, 64, "gate_sandwich_dropout")
    ref = R.resid_case_fwd(R.REF, c)
    w = _worst(R.resid_case_bwd(ar, c, ref, prefill=False), R.resid_case_bwd(R.REF, c, ref))
    assert w["dw_b"] > 1.0 and w["dgate"] > 1.0 and w["dbranch"] <= 1.0, w
    c = R.qk_case("gauss", B, L, 64, 32)
    ref = R.qk_case_fwd(R.REF, c)
    w = _worst(R.qk_case_bwd(ar, c, ref, prefill=False), R.qk_case_bwd(R.REF, c, ref))
    assert all(w[k] > 1.0 for k in ("dgq", "dbq", "dgk", "dbk")) and w["dqk"] <= 1.0, w
    ledger.record(TEST, "mutant/assign_not_accumulate", min(w[k] for k in ("dgq", "dbq", "dgk", "dbk")), 1.0, note="must exceed 1")


# ------------------------------------------------------------------------------------------------ SUBS cross-entropy
CE_SPLITS = [(65, 41, 40), (65, 41, 20), (1001, 1001, 1000), (40193, 32001, 32000)]       # (V, Vt, mask_id): one split with mask_id not at Vt - 1


def _ce_ref(family, V, Vt, mask_id, restrict):
    z, x0, xt, modality, g, ld = R.ce_case(family, V, Vt, mask_id)
    valid = R.valid_ids(z.shape[0], V, Vt, mask_id, modality, restrict)
    lse = R.lse64(z, valid, V).to(R.F32)
    return z, x0, xt, modality, g, ld, valid, lse


@pytest.mark.parametrize("family", R.CE_FAMILIES)
@pytest.mark.parametrize("V,Vt,mask_id", CE_SPLITS)
def test_ce_emulations_stay_within_the_bound(V, Vt, mask_id, family):
    worst = 0.0
    for restrict in ((True, False) if V > Vt else (False,)):
        z, x0, xt, modality, g, ld, valid, lse = _ce_ref(family, V, Vt, mask_id, restrict)
        ref = R.subs_ce_bwd(R.REF, z, x0, xt, lse, g, valid, V, mask_id)
        assert torch.isfinite(ref["dlogits"]).all()
        for fast in (False, True):
            got = R.subs_ce_bwd(R.Arith(R.F32, "torch"), z, x0, xt, lse, g, valid, V, mask_id, fast_exp=fast)
            r = R.worst(got["dlogits"], ref["dlogits"], ref["E_dlogits"], True)[0]
            assert r <= 1.0, (restrict, fast, r)
            worst = max(worst, r)
    ledger.check(TEST, f"ce_bwd_emulation/{family}/V{V}_mask{mask_id}", worst, 1.0)


def test_ce_constant_is_the_rule_applied_to_the_measured_ratio():
    worst = 0.0
    for family in R.CE_FAMILIES:
        for V, Vt, mask_id in CE_SPLITS[:3]:
            z, x0, xt, modality, g, ld, valid, lse = _ce_ref(family, V, Vt, mask_id, V > Vt)
            ref = R.subs_ce_bwd(R.REF, z, x0, xt, lse, g, valid, V, mask_id, c=1)
            for fast in (False, True):
                got = R.subs_ce_bwd(R.Arith(R.F32, "torch", round_out=False), z, x0, xt, lse, g, valid, V, mask_id, fast_exp=fast)
                worst = max(worst, R.worst(got["dlogits"], ref["dlogits"], ref["E_dlogits"], False)[0])
    print(f"worst d-logits ratio at c = 1: {worst:.3f}")
    ledger.record(TEST, "ce_c1_worst_ratio", worst)
    c = 1
    while c < 4 * worst:
        c *= 2
    assert c == R.CE_C, worst


@pytest.mark.parametrize("mutant", ["mask_id_admitted", "seam_off_by_one"])
def test_ce_mutants_are_rejected(mutant):
    """forbidden_spikes: +80 on mask_id and on both sides of the modality seam - a leaked column moves the result by O(1)"""
    V, Vt, mask_id = 65, 41, 20
    z, x0, xt, modality, g, ld, valid, lse = _ce_ref("forbidden_spikes", V, Vt, mask_id, True)
    bad_valid = R.valid_ids(z.shape[0], V, Vt, mask_id, modality, True, mutant=mutant)
    ar = R.Arith(R.F32, "torch")
    ref = R.subs_ce_bwd(R.REF, z, x0, xt, lse, g, valid, V, mask_id)
    ok_r = R.worst(R.subs_ce_bwd(ar, z, x0, xt, lse, g, valid, V, mask_id)["dlogits"], ref["dlogits"], ref["E_dlogits"], True)[0]
    bad_r = R.worst(R.subs_ce_bwd(ar, z, x0, xt, lse, g, bad_valid, V, mask_id)["dlogits"], ref["dlogits"], ref["E_dlogits"], True)[0]
    assert ok_r <= 1.0 and bad_r > 1e3, (ok_r, bad_r)
    # the same leak through the full-row log-probabilities: the lse moves by about 80
    want = R.subs_logprobs64(z, xt, valid, V, mask_id)
    leak = R.subs_logprobs64(z, xt, bad_valid, V, mask_id)
    err = (leak - want).abs()
    assert float(err.max()) > 1.0 and not bool((err <= R.LSE_ATOL + R.LSE_RTOL * want.abs()).all())
    ledger.record(TEST, f"mutant/{mutant}/ce_bwd", bad_r, 1.0, note="must exceed 1")


def test_ce_poison_and_window_helpers():
    V, Vt, mask_id = 65, 41, 40
    z, x0, xt, modality, g, ld, valid, lse = _ce_ref("gauss", V, Vt, mask_id, True)
    p = R.ce_poison(z, valid, V)
    assert torch.isnan(p[:, V:]).all() and torch.isnan(p[:, mask_id]).all() and torch.equal(torch.isnan(p[:, :V]), ~valid)
    assert torch.equal(R.lse64(p.nan_to_num(0.0), valid, V), R.lse64(z, valid, V))
    win = R.narrow_window(z.shape[0], ld, Vt, 20)
    assert win[0, :64].all() and not win[0, 64:].any() and win[20, 40:].all() and not win[20, :40].any()
    lp, lse_f = R.subs_ce_fwd64(z, x0, xt, valid, V, mask_id)
    assert float(lp[6]) < -9e5 and (lp[1::2] == 0).all() and (lse_f[1::2] == 0).all()       # x0 = mask_id takes the NEG branch; unmasked rows: log p = 0
    full = R.subs_logprobs64(z, xt, valid, V, mask_id)
    ok = lp > -9e5
    assert torch.allclose(full.gather(1, x0[:, None])[:, 0][ok], lp[ok], atol=1e-12)
