"""udm_subs_ce_bwd (whole-row and narrow) and udm_subs_logprobs (fp32 and bf16 out) of csrc/ce.hip on a real MI355X (pytest -m gpu), element by element
against the fp64 restatement of tests/rowops_ref64.py on its logit families, with NaN in every column the kernels must not depend on: the other modality's
ids under `restrict`, mask_id, and [V, ld) - which the backward has to turn into zeros.  udm_subs_ce_fwd runs on the same inputs once: its log p and lse
against fp64 with the lse bound of test_subs_logp_rows, and its lse against the one the full-row log-probabilities imply.

    d logits (bf16, one rounding)   |got - ref| <= u |ref| + CE_C 2^-23 ((1 + |z - lse|) p + [id == x0]) |g|      (rowops_ref64.subs_ce_bwd; lse: the kernel's own forward lse)
    log-probabilities, fp32         |got - ref| <= 2e-4 + 1e-5 |ref|;   bf16: one rounding on top;   forbidden ids: NEG exactly
Rows: even rows [MASK] rows, odd rows unmasked (zeros); g == 0 on row 4 (zeros); x0 = mask_id on row 6 and x0 in the other modality's range on some rows of
16 .. 22 (the NEG branch: no one-hot term); x0 at the first / last valid id and next to mask_id.  M = 48, ld = V rounded up to 128.
"""
import pytest
import torch

import gemm_ref64 as G
import ledger
import rowops_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "ce_rowwise"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
M = 48
SPLITS = [(65, 41, 40), (65, 41, 20), (1001, 1001, 1000), (40193, 32001, 32000)]       # (V, Vt, mask_id): (65, 41, 20) has mask_id inside the text range
SENTINEL = 7.0


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


def lse_bound(ref):
    return R.LSE_ATOL + R.LSE_RTOL * ref.abs()


def place(t):
    """the [M, ld] logits as a view between NaN guard rows"""
    return G.arena(tuple(t.shape), t.shape[1], BF16, guard_rows=8, device=DEV, fill=t)


CASES = [(V, Vt, m, r) for V, Vt, m in SPLITS for r in (True, False) if V > Vt or not r]      # (a text-only vocabulary has nothing to restrict)


@pytest.mark.parametrize("family", R.CE_FAMILIES)
@pytest.mark.parametrize("V,Vt,mask_id,restrict", CASES, ids=[f"V{v}_Vt{vt}_mask{m}_{'restrict' if r else 'joint'}" for v, vt, m, r in CASES])
def test_subs_ce_rows(K, V, Vt, mask_id, restrict, family):
    z, x0, xt, modality, g, ld = R.ce_case(family, V, Vt, mask_id, M=M)
    assert ld % 128 == 0 and ld >= V
    valid = R.valid_ids(M, V, Vt, mask_id, modality, restrict)
    poisoned = R.ce_poison(z, valid, V)
    masked = xt == mask_id
    d = lambda t: t.to(DEV)
    x0g, xtg, modg, gg = d(x0), d(xt), d(modality), d(g)
    tag = f"{family}/V{V}_mask{mask_id}/{'restrict' if restrict else 'joint'}"

    # forward, once: log p and lse against fp64
    a_in = place(poisoned)
    lp, lse = K.subs_ce_fwd(a_in.view, x0g, xtg, modg, V, Vt, mask_id, restrict)
    lp, lse = lp.cpu(), lse.cpu()
    want_lp, want_lse = R.subs_ce_fwd64(z, x0, xt, valid, V, mask_id)
    assert torch.isfinite(lp).all() and torch.isfinite(lse).all()
    r_lse = float(((lse.double() - want_lse).abs() / lse_bound(want_lse)).max())
    r_lp = float(((lp.double() - want_lp).abs() / lse_bound(want_lp)).max())
    ledger.check(TEST, f"fwd lse {tag}", r_lse, 1.0)
    ledger.check(TEST, f"fwd log_p {tag}", r_lp, 1.0)
    assert torch.equal(lse[~masked], torch.zeros(int((~masked).sum()))) and torch.equal(lp[~masked].double(), want_lp[~masked])
    assert float(lp[6]) < -9e5                                    # x0 = mask_id: the NEG branch
    G.assert_untouched(a_in, "subs_ce_fwd")
    assert torch.equal(a_in.view.cpu().view(torch.int16), poisoned.view(torch.int16)), "the forward changed its logits"

    # full-row log-probabilities, fp32 and bf16
    want_full = R.subs_logprobs64(z, xt, valid, V, mask_id)
    forbidden = want_full == R.NEG
    for dtype in (F32, BF16):
        full = K.subs_logprobs(a_in.view, xtg, modg, V, Vt, mask_id, restrict, out_dtype=dtype).cpu()
        assert tuple(full.shape) == (M, V) and torch.isfinite(full).all()
        E = lse_bound(want_full)
        r = R.worst(full, want_full, E, dtype == BF16)[0]
        ledger.check(TEST, f"logprobs {'fp32' if dtype == F32 else 'bf16'} {tag}", r, 1.0)
        neg = torch.tensor(R.NEG, dtype=F32).to(dtype)
        assert bool((full[forbidden] == neg).all()), "a forbidden id does not hold NEG"
        if dtype == F32:      # the lse the full rows imply (z - log p on a valid id) against the forward's
            col = valid.float().argmax(-1)
            implied = z[:, :V].double().gather(1, col[:, None])[:, 0] - full.double().gather(1, col[:, None])[:, 0]
            assert bool(((implied - lse.double()).abs()[masked] <= lse_bound(want_lse)[masked]).all()), "the forward's lse and the full rows' disagree"
    G.assert_untouched(a_in, "subs_logprobs")

    # backward, whole rows, in place on the poisoned operand
    ref = R.subs_ce_bwd(R.REF, z, x0, xt, lse, g, valid, V, mask_id)
    a_bwd = place(poisoned)
    K.subs_ce_bwd(a_bwd.view, x0g, xtg, modg, d(lse), gg, V, Vt, mask_id, restrict)
    whole = a_bwd.view.cpu()
    r, i = R.worst(whole, ref["dlogits"], ref["E_dlogits"], True)
    ledger.check(TEST, f"bwd d logits {tag}", r, 1.0, note=f"worst at (row, col) = {divmod(i, ld)}")
    assert bool((whole[:, V:] == 0).all()), "[V, ld) must become zeros"
    assert bool((whole[~masked] == 0).all()) and bool((whole[4] == 0).all()), "unmasked rows and rows with g == 0 must be zeros"
    assert bool((whole[:, :V][~valid] == 0).all()), "ids outside the valid range must be zeros"
    G.assert_untouched(a_bwd, "subs_ce_bwd")

    # backward, narrow (head per modality): only the group's columns are written, bit-identical to the whole-row form; the rest keeps its sentinel
    if restrict:
        for n in (0, M // 2 - 4, M):
            win = R.narrow_window(M, ld, Vt, n)
            start = torch.where(win, poisoned, torch.full_like(poisoned, SENTINEL))
            a_n = place(start)
            K.subs_ce_bwd(a_n.view, x0g, xtg, modg, d(lse), gg, V, Vt, mask_id, restrict, narrow_txt_rows=n)
            got = a_n.view.cpu()
            assert torch.equal(got[win].view(torch.int16), whole[win].view(torch.int16)), f"narrow_txt_rows = {n}: differs from the whole-row form inside the window"
            assert bool((got[~win] == SENTINEL).all()), f"narrow_txt_rows = {n}: a column outside the window lost its sentinel"
            ref_n = R.subs_ce_bwd(R.REF, z, x0, xt, lse, g, valid, V, mask_id, window=win, sentinel=torch.full((M, ld), SENTINEL, dtype=F64))
            ledger.check(TEST, f"bwd narrow n{n} {tag}", R.worst(got, ref_n["dlogits"], ref_n["E_dlogits"], True)[0], 1.0)
            G.assert_untouched(a_n, f"subs_ce_bwd narrow {n}")
