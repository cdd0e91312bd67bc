"""udm_nucleus_sample_rows and udm_ar_nucleus_rows (csrc/nucleus.hip) on a real MI355X (pytest -m gpu) against the fp64 reference of tests/nucleus_ref64.py.

Every operand sits in a NaN arena with guard rows, every id the kernel must not depend on (mask_id, the other modality under `restrict`, [V, ld)) holds NaN
- in the logits, the unconditional logits and the uniforms - except in the `spikes` family, whose forbidden ids carry finite +80 spikes.  Per row:
    kept count    accepted by nucleus_ref64.Ref.accepts (the exact prefix for some budget within delta of the requested one); no row is excluded
    token         with replayed uniforms, the fp64 race over the kernel's own (validated) prefix; rows whose two best race values are closer than 2^-18
                  relative are left out, at most 1 % of the rows (tests/test_nucleus_ref64.py checks the same seeds on the CPU)
    log p_1       |got - ref| <= 2e-4 + 1e-5 |ref|, the bound of udm_subs_logp_rows
    a second launch is bit-identical; nothing outside the outputs changes
Philox draws: 32768 identical rows, Pearson's statistic below the 1 - 1e-6 quantile of chi-square.
"""
import pytest
import torch

import gemm_ref64 as G
import nucleus_ref64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENT = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


class IntGuard:
    """an int64 [n] output between sentinel guards"""

    def __init__(self, n, g=16):
        self.raw = torch.full((n + 2 * g,), SENT, dtype=torch.int64, device=DEV)
        self.view, self.n, self.g = self.raw[g:g + n], n, g

    def untouched(self):
        return bool((self.raw[:self.g] == SENT).all()) and bool((self.raw[self.g + self.n:] == SENT).all())


def _operands(c):
    """arenas of the case's operands, poisoned"""
    M, V, ld = c["M"], c["V"], c["ld"]
    finite = c["family"] == "spikes"
    pz = N.poison(c["zc"], c["valid"], V, keep_finite=finite)
    a = {"zc": G.arena((M, ld), ld, BF16, guard_rows=8, device=DEV, fill=pz), "pz": pz, "zu": None,
         "u": G.arena((M, ld), ld, F32, guard_rows=8, device=DEV, fill=N.poison(c["u"], c["valid"], V))}
    if c["zu"] is not None:
        a["pzu"] = N.poison(c["zu"], c["valid"], V, keep_finite=finite)
        a["zu"] = G.arena((M, ld), ld, BF16, guard_rows=8, device=DEV, fill=a["pzu"])
    return a


def _raw_call(K, c, a, rule, seed=0, use_u=True):
    from unidisc_amd import _lib

    M, V = c["M"], c["V"]
    inv_t, budget = N.RULES[rule]
    tok, keep = IntGuard(M), IntGuard(M)
    logp = G.arena((1, M), M, F32, guard_rows=4, device=DEV).poison()
    w = c["w"].to(DEV) if c["w"] is not None else None
    mod = c["modality"].to(DEV)
    _lib.call("udm_nucleus_sample_rows", K._p(a["zc"].view), K._p(a["zu"].view) if a["zu"] is not None else None, K._p(w), c["ld"], K._p(mod),
              K._p(a["u"].view) if use_u else None, c["ld"], seed, inv_t, budget, K._p(tok.view), K._p(logp.view), K._p(keep.view), M, V, c["Vt"], c["mask_id"],
              1 if c["restrict"] else 0, K._s())
    torch.cuda.synchronize()
    assert tok.untouched() and keep.untouched(), "an int64 output was written outside its rows"
    G.assert_untouched(logp, "out_logp")
    for k in ("zc", "zu", "u"):
        if a[k] is not None:
            G.assert_untouched(a[k], k)
    assert torch.equal(a["zc"].view.cpu().view(torch.int16), a["pz"].view(torch.int16)), "the logits changed"
    return tok.view.cpu(), logp.view[0].cpu(), keep.view.cpu()


def _check(c, ref, tok, logp, keep, tag):
    M, V = c["M"], c["V"]
    assert bool(((tok >= 0) & (tok < V)).all()), tag
    assert bool(c["valid"].gather(1, tok[:, None]).all()), f"{tag}: a forbidden id was drawn"
    bad = ref.judge(keep, tok, c["u"])
    assert bad == [], f"{tag}: {bad}"
    want = ref.logp1.gather(1, tok[:, None])[:, 0]
    err = (logp.double() - want).abs()
    assert bool((err <= N.LSE_ATOL + N.LSE_RTOL * want.abs()).all()), f"{tag}: log p_1 off by {float(err.max())}"
    if c["family"] == "flat" and c["zu"] is None:            # (guidance mixes noise in: no longer flat)
        fl, clear = N.flat_floor(ref)
        assert torch.equal(keep[clear], fl[clear]), f"{tag}: flat rows keep {keep.tolist()[:4]}, floor {fl.tolist()[:4]}"
        first = [c["valid"][r].nonzero()[:, 0][:int(keep[r])] for r in range(M)]
        assert all(int(tok[r]) in first[r].tolist() for r in range(min(M, 16))), f"{tag}: a flat row drew outside its first ids"
    if c["family"] in ("peak", "neg300"):
        assert bool((keep == ref.n).all()), tag
    if c["family"] == "peak":
        assert torch.equal(tok[keep == 1], ref.order[keep == 1, 0]), f"{tag}: not the first index of the tied peak"


@pytest.mark.parametrize("rule", sorted(N.RULES))
@pytest.mark.parametrize("V,Vt,mask_id,M,restrict,guided", N.GPU_CASES,
                         ids=[f"V{v}_M{m}_{'restrict' if r else 'joint'}_{'cfg' if g else 'plain'}" for v, _, _, m, r, g in N.GPU_CASES])
def test_nucleus_rows(K, V, Vt, mask_id, M, restrict, guided, rule):
    inv_t, budget = N.RULES[rule]
    for family in N.FAMILIES:
        c = N.case(family, V, Vt, mask_id, M, restrict=restrict, guided=guided)
        ref = N.Ref(c["zc"], c["zu"], c["w"], c["valid"], inv_t, budget, V)
        a = _operands(c)
        tag = f"{family}/{rule}"
        tok, logp, keep = _raw_call(K, c, a, rule)
        _check(c, ref, tok, logp, keep, tag)
        # the wrapper, a second launch: bit-identical
        t2, l2, k2 = K.nucleus_sample_rows(a["zc"].view, V, Vt, mask_id, inv_temperature=inv_t, budget=budget, modality=c["modality"].to(DEV), restrict=c["restrict"],
                                           u=a["u"].view, logits_u=a["zu"].view if guided else None, w=c["w"].to(DEV) if guided else None, want_keep=True)
        assert torch.equal(t2.cpu(), tok) and torch.equal(k2.cpu(), keep) and torch.equal(l2.cpu().view(torch.int32), logp.view(torch.int32)), f"{tag}: second launch"


def test_degenerate_shapes(K):
    V, ld = 64, 72
    z = torch.randn(4, ld).to(BF16)
    # Vt = 1: a text row has the single valid id 0 under `restrict`
    tok, logp, keep = K.nucleus_sample_rows(z.to(DEV), V, 1, 5, inv_temperature=1.0, budget=0.855, modality=torch.zeros(4, dtype=torch.int64, device=DEV),
                                            restrict=True, want_keep=True)
    assert tok.tolist() == [0] * 4 and keep.tolist() == [1] * 4 and float(logp.abs().max()) == 0.0
    e = torch.empty(0, ld, dtype=BF16, device=DEV)
    tok, logp = K.nucleus_sample_rows(e, V, 41, 40, inv_temperature=1.0, budget=0.855)
    assert tok.numel() == 0 and logp.numel() == 0
    big = torch.zeros(1, 65544, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="held in registers"):
        K.nucleus_sample_rows(big, 65537, 65537, 65536, inv_temperature=1.0, budget=0.855)
    tok, _, keep = K.nucleus_sample_rows(big[:, :65536], 65536, 65536, 65535, inv_temperature=1.0, budget=0.5, want_keep=True)      # the largest supported V
    assert int(keep[0]) == 32767 and 0 <= int(tok[0]) < 32767


def test_philox_draws_follow_the_kept_distribution(K):
    inv_t, budget = N.RULES["batch"]
    V, ld = N.CHI_V, N.CHI_V + 8
    for i, row in enumerate(N.chi_rows()):
        valid = torch.ones(1, V, dtype=torch.bool)
        ref = N.Ref(row[None], None, None, valid, inv_t, budget, V)
        n = int(ref.n[0])
        kept = ref.order[0, :n]
        expect = ref.p[0, kept] / ref.S[0, n - 1]
        z = torch.full((N.CHI_ROWS, ld), float("nan"), dtype=BF16)
        z[:, :V] = row
        zg = z.to(DEV)
        draw = lambda seed: K.nucleus_sample_rows(zg, V, V, V, inv_temperature=inv_t, budget=budget, seed=seed, want_keep=True)      # mask_id = V: no id is masked
        tok, logp, keep = draw(1234 + i)
        assert bool((keep == n).all())
        stat, outside = N.pearson(tok.cpu(), expect, kept)
        q = N.chi2_quantile(n - 1)
        print(f"distribution {i}: kept {n}, Pearson {stat:.2f}, quantile {q:.2f}")
        assert outside == 0, f"{outside} tokens outside the kept set"
        assert stat < q, (i, stat, q)
        again = draw(1234 + i)[0]
        other = draw(99 + i)[0]
        assert torch.equal(again, tok) and not torch.equal(other, tok)
        assert float((tok[1:] != tok[:-1]).float().mean()) > 0.3      # rows draw independently


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("R,V,Vt,mask_id", [(1, 1000, 611, 600), (8, 48385, 32001, 48384), (64, 1000, 611, 600)])
def test_ar_nucleus_rows(K, R, V, Vt, mask_id, guided):
    """the AR entry: the rows entry's token on the same inputs (scalar w, uniforms at a column offset), and the write-back rules of udm_ar_sample_rows"""
    inv_t, budget = N.RULES["ar"]
    L, pos, step, col0 = 12, 5, 4, 16
    for family in ("gauss", "plateaus", "spikes"):
        c = N.case(family, V, Vt, mask_id, R, restrict=True, guided=guided, seed=1)
        ld = c["ld"]
        wv = 1.5
        if guided:
            c["w"] = torch.full((R,), wv, dtype=F32)
        ref = N.Ref(c["zc"], c["zu"], c["w"], c["valid"], inv_t, budget, V)
        finite = family == "spikes"
        rows2 = 2 * R if guided else R
        both = torch.zeros(rows2, ld, dtype=BF16)
        both[:R] = N.poison(c["zc"], c["valid"], V, keep_finite=finite)
        if guided:
            both[R:] = N.poison(c["zu"], c["valid"], V, keep_finite=finite)
        a_l = G.arena((rows2, ld), ld, BF16, guard_rows=8, device=DEV, fill=both)
        a_u = G.arena((R, ld), col0 + ld + 8, F32, guard_rows=8, device=DEV, fill=N.poison(c["u"], c["valid"], V), col0=col0)
        modality = torch.zeros(R, L, dtype=torch.int64)
        modality[:, pos] = c["modality"]
        modality[:, pos - 1] = 1 - c["modality"]            # a kernel that reads the wrong column restricts to the wrong range
        x = torch.full((R, L), 7, dtype=torch.int64)
        x0 = torch.randint(0, V, (R, L))
        unmask = torch.zeros(R, L, dtype=torch.bool)
        unmask[::3, pos] = True
        unmask[:, pos + 1] = True
        xg, ids = x.to(DEV), IntGuard(rows2)
        w = torch.full((4,), wv, dtype=F32, device=DEV)
        K.ar_nucleus_rows(a_l.view, xg, pos, V, Vt, mask_id, inv_temperature=inv_t, budget=budget, step=step, modality=modality.to(DEV), restrict=True, u=a_u.buf[
            8 * a_u.ld:(8 + R) * a_u.ld].view(R, a_u.ld), u_col0=col0, x0=x0.to(DEV), x0_unmask=unmask.to(DEV), next_ids=ids.view,
            logits_u=a_l.view[R:] if guided else None, w=w if guided else None, rows=R)
        torch.cuda.synchronize()
        G.assert_untouched(a_l, "logits"), G.assert_untouched(a_u, "u")
        assert ids.untouched()
        got = xg.cpu()
        keepcol = torch.ones(L, dtype=torch.bool)
        keepcol[pos] = False
        assert bool((got[:, keepcol] == 7).all()), "another column of x was written"
        # the rows entry on the same operands: its validated prefix, its token
        tok, logp, keep = K.nucleus_sample_rows(a_l.view[:R], V, Vt, mask_id, inv_temperature=inv_t, budget=budget, modality=c["modality"].to(DEV), restrict=True,
                                                u=a_u.view, logits_u=a_l.view[R:] if guided else None, w=c["w"].to(DEV) if guided else None, want_keep=True)
        _check(c, ref, tok.cpu(), logp.cpu(), keep.cpu(), f"{family}/ar")
        want = torch.where(unmask[:, pos], x0[:, pos], tok.cpu())
        assert torch.equal(got[:, pos], want), family
        nid = ids.view.cpu()
        assert torch.equal(nid[:R], want)
        if guided:
            assert torch.equal(nid[R:], torch.where(unmask[:, pos], torch.full_like(want, mask_id), want))
        # Philox: reproducible per (seed, step), different across steps, tokens inside the validated prefix
        def free(step_, seed_):
            xs = x.to(DEV)
            K.ar_nucleus_rows(a_l.view, xs, pos, V, Vt, mask_id, inv_temperature=inv_t, budget=budget, step=step_, modality=modality.to(DEV), restrict=True, seed=seed_,
                              logits_u=a_l.view[R:] if guided else None, w=w if guided else None, rows=R)
            return xs[:, pos].cpu()
        t1, t1b = free(3, 77), free(3, 77)
        assert torch.equal(t1, t1b)
        rank = torch.empty_like(ref.order)
        rank.scatter_(1, ref.order, torch.arange(V)[None].expand(R, V))
        assert bool((rank.gather(1, t1[:, None])[:, 0] < keep.cpu()).all()), f"{family}: a Philox token outside the kept prefix"
        if R >= 8 and family == "gauss":
            assert not torch.equal(free(4, 77), t1) and not torch.equal(free(3, 78), t1)
