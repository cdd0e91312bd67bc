"""The two likelihood-scoring kernels of csrc/ce.hip on a real MI355X (pytest -m gpu).

`udm_subs_logp_rows` against an fp64 restatement on the same bf16 logits - z = (1 + w) l_c - w l_u, log-sum-exp over the ids valid for the row's modality
without mask_id, z[x0] - lse - with atol = 2e-4 (1 + 2 max w), rtol = 1e-5: the bound of test_subs_ce (tests/test_gpu_kernels.py) scaled by the factor by
which guidance enlarges |z| (|z| <= (1 + 2 w) max(|l_c|, |l_u|): the fp32 rounding of z and of exp / log arguments grows with it).
`udm_likelihood_scores` against fp64 with the summation bound (n + 2) 2^-24 sum|term| / count: one rounding per product, n - 1 per sum, one for the division.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(65, 41), (1001, 1001), (40193, 32001)]
M = 48
SENTINEL = 16


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels

    return kernels


def _case(V, Vt, restrict):
    """Rows 0..: the required adversarial rows, then random ones.  Returns l_c, l_u (bf16 [M, ld], clean: finite everywhere), x0, modality, w, mask_id."""
    g = torch.Generator().manual_seed(1000 + V)
    ld = (V + 127) // 128 * 128
    mask_id = Vt - 1
    two = V > Vt
    lc = torch.zeros(M, ld, dtype=torch.bfloat16)
    lu = torch.zeros(M, ld, dtype=torch.bfloat16)
    lc[:, :V] = (2.0 * torch.randn(M, V, generator=g)).bfloat16()
    lu[:, :V] = (2.0 * torch.randn(M, V, generator=g)).bfloat16()
    modality = (torch.arange(M) % 4 >= 2).long() if two else torch.zeros(M, dtype=torch.long)
    lo = torch.where(modality == 1, Vt, 0) if restrict else torch.zeros(M, dtype=torch.long)     # first id of the row's valid range
    # a valid x0 per row: inside the row's modality (valid with and without the restriction), never mask_id
    x0 = torch.where(modality == 1, torch.randint(Vt, max(V, Vt + 1), (M,), generator=g), torch.randint(0, Vt - 1, (M,), generator=g))
    for r in (0, 2):                                   # +60 spikes at different ids in l_c and l_u (a text row and an image row)
        a, b = int(lo[r]) + 3, int(lo[r]) + 11
        lc[r, a] += 60.0
        lu[r, b] += 60.0
    for r in (1, 3):                                   # all valid logits equal: lse = z + log n
        lc[r, :V] = 1.25
        lu[r, :V] = -0.5
    for r in (4, 6):                                   # the row's largest logit at mask_id: excluded always
        lc[r, mask_id] = 90.0
        lu[r, mask_id] = -90.0
    if two:
        for r in (5, 7):                               # the row's largest logit in the OTHER modality: excluded under the restriction only
            other = 2 if modality[r] == 1 else Vt + 2
            lc[r, other] = 70.0
            lu[r, other] = -70.0
    for r in (8, 10):                                  # x0 at the first / last valid id of the row's modality
        x0[r] = Vt if modality[r] == 1 else 0
    for r in (9, 11):
        x0[r] = V - 1 if modality[r] == 1 else Vt - 2
    if two and Vt % 8 != 0:                            # x0 at Vt: the image range starts inside a 16-byte group
        x0[14] = Vt
        assert modality[14] == 1
    x0[12] = mask_id                                   # an invalid x0: the NEG convention of subs_ce_fwd (z[x0] := -1e6)
    w = 3.0 * torch.rand(M, generator=g)
    w[::5] = 0.0
    w[1] = 3.0
    return lc, lu, x0, modality, w, mask_id, ld


def _valid(V, Vt, mask_id, modality, restrict):
    ar = torch.arange(V)[None]
    v = torch.where((modality == 1)[:, None], ar >= Vt, ar < Vt) if restrict else torch.ones(modality.shape[0], V, dtype=torch.bool)
    v = v.clone()
    v[:, mask_id] = False
    return v


def _fp64(lc, lu, w, x0, valid, V):
    z = lc[:, :V].double()
    if w is not None:
        wd = w.double()[:, None]
        z = (1 + wd) * z - wd * lu[:, :V].double()
    z = z.masked_fill(~valid, float("-inf"))
    zx = z.gather(1, x0[:, None])[:, 0]
    zx = torch.where(torch.isinf(zx), torch.full_like(zx, -1e6), zx)
    return zx - torch.logsumexp(z, -1)


def _poison(t, valid, V):
    """NaN in every column the result must not depend on: [V, ld), mask_id and (under the restriction) the other modality's ids"""
    p = t.clone()
    p[:, V:] = float("nan")
    p[:, :V] = torch.where(valid, p[:, :V], torch.full_like(p[:, :V], float("nan")))
    return p


def _launch(K, lc, lu, w, x0, modality, V, Vt, mask_id, restrict):
    """the C entry point on a caller-owned output with 16 sentinel entries past M"""
    from unidisc_amd import _lib

    out = torch.full((M + SENTINEL,), -12345.0, dtype=torch.float32, device=DEV)
    _lib.call("udm_subs_logp_rows", K._p(lc), K._p(lu), K._p(w), lc.stride(0), K._p(x0), K._p(modality), K._p(out), M, V, Vt, mask_id, 1 if restrict else 0,
              K._s())
    out = out.cpu()
    assert torch.all(out[M:] == -12345.0), "udm_subs_logp_rows wrote past its M outputs"
    return out[:M]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("restrict", [True, False])
@pytest.mark.parametrize("V,Vt", SHAPES)
def test_subs_logp_rows(K, V, Vt, restrict, guided):
    lc, lu, x0, modality, w, mask_id, ld = _case(V, Vt, restrict)
    valid = _valid(V, Vt, mask_id, modality, restrict)
    want = _fp64(lc, lu, w if guided else None, x0, valid, V)
    d = lambda t: t.to(DEV)
    args = (d(x0), d(modality), V, Vt, mask_id, restrict)
    got = _launch(K, d(lc), d(lu) if guided else None, d(w) if guided else None, *args)
    assert torch.isfinite(got).all()
    atol = 2e-4 * (1 + 2 * (float(w.max()) if guided else 0.0))
    err = (got.double() - want).abs()
    print(f"V={V} Vt={Vt} restrict={restrict} guided={guided}: max |log_p - fp64| = {float(err[want > -1e5].max()):.3e} (atol {atol:.1e})")
    assert (err <= atol + 1e-5 * want.abs()).all(), (int(err.argmax()), float(err.max()))
    # known answers inside the case: equal valid logits -> log p = -log n
    n_valid = valid.sum(-1).double()
    for r in (1, 3):
        assert abs(float(got[r]) + float(torch.log(n_valid[r]))) <= atol
    # NaN wherever the result must not look: unchanged (bit for bit) and finite
    got_p = _launch(K, d(_poison(lc, valid, V)), d(_poison(lu, valid, V)) if guided else None, d(w) if guided else None, *args)
    assert torch.isfinite(got_p).all() and torch.equal(got_p, got)
    # the wrapper returns the same values
    assert torch.equal(K.subs_logp_rows(d(lc), d(x0), d(modality), V, Vt, mask_id, restrict, logits_u=d(lu) if guided else None, w=d(w) if guided else None).cpu(), got)
    if not guided:   # w NULL: bit-identical to udm_subs_ce_fwd's log_p of the same all-[MASK] rows (one shared loop)
        lp, _ = K.subs_ce_fwd(d(lc), d(x0), torch.full((M,), mask_id, dtype=torch.int64, device=DEV), d(modality), V, Vt, mask_id, restrict)
        assert torch.equal(lp.cpu(), got)
    else:            # rows with w = 0 are the unguided rows, whatever l_u holds
        plain = _launch(K, d(lc), None, None, *args)
        zero = w == 0
        assert zero.sum() >= 5 and ((got[zero].double() - plain[zero].double()).abs() <= 2e-4 + 1e-5 * plain[zero].abs().double()).all()


def test_subs_logp_rows_refuses_half_a_guidance_pair(K):
    lc, lu, x0, modality, w, mask_id, ld = _case(65, 41, True)
    with pytest.raises(ValueError, match="guidance"):
        K.subs_logp_rows(lc.to(DEV), x0.to(DEV), modality.to(DEV), 65, 41, mask_id, True, logits_u=lu.to(DEV))
    assert K.subs_logp_rows(lc[:0].to(DEV), x0[:0].to(DEV), modality[:0].to(DEV), 65, 41, mask_id, True).numel() == 0


def test_likelihood_scores(K):
    """S = 6, L = 32: a sample without rows (0 / count), one with every row, one with valid_count = 0 (NaN); fp64 with the summation bound; two launches
    bit-identical."""
    S, L = 6, 32
    g = torch.Generator().manual_seed(77)
    keep = torch.rand(S, L, generator=g) < 0.4
    keep[1] = False                                         # no rows, count > 0: 0 / count
    keep[2] = True                                          # every row
    keep[4] = False                                         # nothing but padding: no rows, count = 0 -> NaN
    rows = keep.reshape(-1).nonzero().reshape(-1)
    n = rows.numel()
    log_p = -(6.0 * torch.rand(n, generator=g) + 0.01)
    log_p[3] = -1e6 - 4.0                                   # an invalid-x0 row (NEG convention) in sample 0
    w_std = 1.0 / (0.05 + torch.rand(S, generator=g))
    count = torch.tensor([32.0, 17.0, 32.0, 29.0, 0.0, 8.0])
    d = lambda t: t.to(DEV)
    wgt, unw = K.likelihood_scores(d(log_p), d(rows), d(w_std), d(count), L)
    wgt2, unw2 = K.likelihood_scores(d(log_p), d(rows), d(w_std), d(count), L)
    assert torch.equal(wgt.view(torch.int32), wgt2.view(torch.int32)) and torch.equal(unw.view(torch.int32), unw2.view(torch.int32))
    wgt, unw = wgt.cpu(), unw.cpu()
    seg = rows // L
    for s in range(S):
        terms = -log_p[seg == s].double()
        ns = terms.numel()
        if count[s] == 0:
            assert ns == 0 and torch.isnan(unw[s]) and torch.isnan(wgt[s])     # 0 / 0, as the reference's
            continue
        want_u, want_w = terms.sum() / count[s].double(), (terms * w_std[s].double()).sum() / count[s].double()
        bound_u = (ns + 2) * 2.0 ** -24 * terms.abs().sum() / count[s].double()
        bound_w = (ns + 2) * 2.0 ** -24 * (terms.abs() * w_std[s].double()).sum() / count[s].double()
        assert abs(float(unw[s]) - float(want_u)) <= float(bound_u), (s, float(unw[s]), float(want_u))
        assert abs(float(wgt[s]) - float(want_w)) <= float(bound_w), (s, float(wgt[s]), float(want_w))
    assert float(unw[1]) == 0.0 and float(wgt[1]) == 0.0 and int((seg == 2).sum()) == L
    # no rows at all
    e = torch.empty(0, device=DEV)
    wgt_e, unw_e = K.likelihood_scores(e, e.long(), d(w_std), d(count), L)
    assert torch.all(unw_e.cpu()[count > 0] == 0) and torch.isnan(unw_e.cpu()[4])
