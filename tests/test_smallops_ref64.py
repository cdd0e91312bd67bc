"""The reference of tests/test_gpu_smallops_exact.py on its own (CPU): the IEEE statements of the casts agree with torch's own casts on the `edges` family, which
holds what it promises; the `ints` families are exact in fp32 in two orders and the `gauss` families stay inside gamma_n sum|terms|; the fp32 restatements of
the timestep embedding and of SiLU lie inside their intervals, W is measured and equals the constants of tests/smallops_ref64.py, the share of elements with
more than one allowed value is at most 2 % where capped - and the comparators reject every mutant of the list."""
import math

import pytest
import torch

import fake_kernels
import gemm_ref64 as G
import smallops_ref64 as S

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ rounding
def test_rounding_helpers():
    assert float(torch.tensor(2.0 ** -140, dtype=F64).to(F32)) == 2.0 ** -140                       # this host keeps subnormals: the statements rely on it
    x = torch.cat([torch.randn(20000) * 3, S.edges(4099, 3, 1 / 8)])
    fin = ~torch.isnan(x)
    assert S.mismatches(S.round_bf16_64(x.double()), S.rne(x))[0] == 0                               # the interval rounding agrees with the bit statement
    assert S.mismatches(S.rne(x)[fin], x[fin].to(BF16))[0] == 0                                      # ... and that with torch's cast
    assert torch.isnan(S.rne(torch.tensor([float("nan")]))).all()
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 2.0 ** -134, 3 * 2.0 ** -134, 3.39e38, 3.4e38], dtype=F64)
    assert S.round_bf16_64(t).tolist() == [1.0 + 2.0 ** -7, 1.0, 0.0, 2.0 ** -132, float(torch.tensor(3.39e38).to(BF16)), float("inf")]
    assert S.mismatches(torch.tensor([float("nan"), 0.0]), torch.tensor([float("nan"), -0.0]))[0] == 0
    assert S.mismatches(torch.tensor([float("nan"), 1.0]), torch.tensor([1.0, float("nan")]))[0] == 2


# ------------------------------------------------------------------------------------------------ casts
@pytest.mark.parametrize("scale", S.SCALES)
def test_edges_family(scale):
    for n in S.CAST_N:
        x = S.edges(n, 1, scale)
        share, both = S.tie_share(x)
        assert share >= 0.25, (n, share)
        if n >= 1023:
            u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            low, mag = u & 0xFFFF, u & 0x7FFFFFFF
            r = S.rne(x).double()
            assert both
            assert bool(((low == 0x8001) & torch.isfinite(x)).any()) and bool(((low == 0x7FFF) & torch.isfinite(x)).any())
            assert bool((u == 0).any()) and bool((u == 0x80000000).any())
            assert bool(((mag > 0) & (mag < 0x800000)).any()) and bool((mag == 0x7F7F0000).any())
            assert bool((torch.isfinite(x) & torch.isinf(r)).any()) and bool((x == float("inf")).any()) and bool((x == -float("inf")).any())
            assert bool(torch.isnan(x).any()) and bool(S.cast_subnormals(x, scale).any())
    # the scaled products: `scaled_tie_values` searches every finite bf16; what it finds is a tie and is in the family
    st, exists = S.scaled_tie_values(scale)
    assert exists == (scale in (1.0 / 6.0, 1.0 / 8.0))
    if exists:
        ps = (st * S.f32(scale)).to(F32)
        assert bool(((ps.view(torch.int32).to(torch.int64) & 0xFFFF) == 0x8000).all()) and float(ps.abs().max()) < S.MIN_NORMAL    # all of them below the normals
        x = S.edges(4099, 1, scale)
        px = (S.rne(x).double() * S.f32(scale)).to(F32)
        assert int((torch.isfinite(px) & (px != 0) & ((px.view(torch.int32).to(torch.int64) & 0xFFFF) == 0x8000)).sum()) >= 100
    elif scale != 1.0:
        assert st.numel() == 4                                                                       # 1/3: no product is a tie; the nearest mantissas stand in


@pytest.mark.parametrize("scale", S.SCALES)
def test_cast_statements_agree_with_torch(scale):
    """the bit statement against torch's IEEE ops on this host: two derivations of the same value"""
    for n in (5, 4099):
        x = torch.cat([S.edges(n, 2, scale), S.gauss((n,), 2)])
        ok = ~torch.isnan(x)
        s = torch.tensor(scale, dtype=F32)
        want = x.to(BF16) if scale == 1.0 else (x.to(BF16).float() * s).to(BF16)
        got = S.cast_f32_bf16_ref(x, scale)
        assert S.mismatches(got[ok], want[ok])[0] == 0 and bool(torch.isnan(got[~ok].float()).all())
        b = S.edges_bf16(n, 2)
        assert S.mismatches(S.cast_bf16_f32_ref(b, scale), b.float() * s)[0] == 0


def test_cast_mutants_rejected():
    x = S.edges(4099, 1, 1.0 / 3.0)
    ref1, ref3 = S.cast_f32_bf16_ref(x, 1.0), S.cast_f32_bf16_ref(x, 1.0 / 3.0)
    for m in ("half_away", "truncate"):
        assert S.mismatches(S.cast_f32_bf16_ref(x, 1.0, mutant=m), ref1)[0] > 0
        assert S.mismatches(S.cast_f32_bf16_ref(x, 1.0 / 3.0, mutant=m), ref3)[0] > 0
    assert S.mismatches(S.cast_f32_bf16_ref(x, 1.0 / 3.0, mutant="scale_first"), ref3)[0] > 0       # "round then scale" against "scale then round"
    g = S.gauss((4099,), 1)
    assert S.mismatches(S.cast_f32_bf16_ref(g, 1.0 / 3.0, mutant="scale_first"), S.cast_f32_bf16_ref(g, 1.0 / 3.0))[0] > 0
    assert S.mismatches(S.cast_f32_bf16_ref(g, 1.0 / 8.0, mutant="scale_first"), S.cast_f32_bf16_ref(g, 1.0 / 8.0))[0] == 0   # what a power of two cannot tell


# ------------------------------------------------------------------------------------------------ embedding
V, HOT = S.EMB_V, S.EMB_HOT
_emb_case = S.emb_case


def _emb_fp32(ids, mod, dx, dE0, dEm0, reverse):
    """fp32 scatter-adds in two orders: torch's index_add_, or row by row from the last row"""
    ok = (ids >= 0) & (ids < dE0.shape[0])
    m = (mod != 0).long()
    if not reverse:
        return dE0.clone().index_add_(0, ids[ok], dx[ok]), dEm0.clone().index_add_(0, m, dx)
    dE, dEm = torch.zeros_like(dE0), torch.zeros_like(dEm0)
    for r in range(ids.numel() - 1, -1, -1):
        if ok[r]:
            dE[ids[r]] += dx[r]
        dEm[m[r]] += dx[r]
    return dE + dE0, dEm + dEm0


@pytest.mark.parametrize("d", (4, 192, 1028))
@pytest.mark.parametrize("M", S.EMB_BWD_M)
def test_embedding_bwd_families(d, M):
    for share in (0.0, 0.5, 1.0):
        ids, mod, dx, dE0, dEm0, f = _emb_case("ints", d, M, share)
        ref = S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0)
        assert S.partial_sums_exact(ref["A_dE"], f) and S.partial_sums_exact(ref["A_dEm"], f)       # no partial sum of any order leaves the 24-bit integers
        for rev in (False, True):
            dE, dEm = _emb_fp32(ids, mod, dx, dE0, dEm0, rev)
            assert S.mismatches(dE, ref["dE"])[0] == 0 and S.mismatches(dEm, ref["dEm"])[0] == 0
        ids, mod, dx, dE0, dEm0, _ = _emb_case("gauss", d, M, share)
        ref = S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0)
        for rev in (False, True):
            dE, dEm = _emb_fp32(ids, mod, dx, dE0, dEm0, rev)
            assert S.sum_ratio(dE, ref["dE"], ref["A_dE"], ref["n_dE"]) <= 1 and S.sum_ratio(dEm, ref["dEm"], ref["A_dEm"], ref["n_dEm"]) <= 1


def test_embedding_exactness_at_every_gpu_shape():
    for d in S.EMB_BWD_D:
        for M in S.EMB_BWD_M:
            ids, mod, dx, dE0, dEm0, f = _emb_case("ints", d, M, 1.0)
            ref = S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0)
            assert S.partial_sums_exact(ref["A_dE"], f) and S.partial_sums_exact(ref["A_dEm"], f)
            assert torch.equal(ref["dE"].to(F32).double(), ref["dE"])


@pytest.mark.parametrize("family", ("ints", "gauss"))
def test_embedding_mutants_rejected(family):
    d, M = 192, 1000

    def rejected(ref, mut):
        if family == "ints":
            return S.mismatches(mut["dE"], ref["dE"])[0] + S.mismatches(mut["dEm"], ref["dEm"])[0] > 0
        return max(S.sum_ratio(mut["dE"], ref["dE"], ref["A_dE"], ref["n_dE"]), S.sum_ratio(mut["dEm"], ref["dEm"], ref["A_dEm"], ref["n_dEm"])) > 1

    ids, mod, dx, dE0, dEm0, _ = _emb_case(family, d, M, 0.5)
    ref = S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0)
    assert not rejected(ref, ref)
    for m in ("drop_block_last_row", "hot_twice", "modality_swapped", "clamp_out_of_range"):
        assert rejected(ref, S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0, mutant=m, hot_id=HOT)), m
    ids2, dx2 = S.cancelling_hot_block(ids, dx, HOT, V)
    ref2 = S.embedding_bwd_ref(ids2, dx2, dE0, mod, dEm0)
    assert S.mismatches(ref2["dE"][HOT], dE0[HOT])[0] == 0                                           # the cancelled row keeps its starting value
    assert rejected(ref2, S.embedding_bwd_ref(ids2, dx2, dE0, mod, dEm0, mutant="cancelled_hot_garbage", hot_id=HOT))


def test_embedding_fwd_statement_and_fake_kernels_contract():
    """forward clamps, backward drops - in the statement and in tests/fake_kernels.py alike"""
    M, d = 9, 8
    ids = S.make_ids(M, V, 1, hot_id=HOT, hot_share=0.5)
    assert {-1, -100, V, V + 7} <= set(ids.tolist())
    mod = S.make_modality(M, 1)
    E, Em = S.gauss((V, d), 1), S.gauss((2, d), 2)
    ref = S.embedding_fwd_ref(ids, E, mod, Em)
    assert torch.equal(ref[1], E[0] + Em[int(mod[1] != 0)]) and torch.equal(ref[M - 1], E[V - 1] + Em[int(mod[M - 1] != 0)])
    assert torch.equal(fake_kernels.embedding_fwd(ids, E, mod, Em), ref) and torch.equal(fake_kernels.embedding_fwd(ids, E), S.embedding_fwd_ref(ids, E))
    out = torch.full((M, d), float("nan"))
    assert fake_kernels.embedding_fwd(ids, E, mod, Em, out=out) is out and torch.equal(out, ref)
    dx, f = S.ints(M, d, 3)
    dE0, dEm0 = S.ints_like((V, d), f, 4).to(F32), S.ints_like((2, d), f, 5).to(F32)
    r = S.embedding_bwd_ref(ids, dx.to(F32), dE0, mod, dEm0)
    for hot in (HOT, -1, V):
        dE, dEm = dE0.clone(), dEm0.clone()
        fake_kernels.embedding_bwd(ids, dx.to(F32), dE, hot, mod, dEm)
        assert S.mismatches(dE, r["dE"])[0] == 0 and S.mismatches(dEm, r["dEm"])[0] == 0


# ------------------------------------------------------------------------------------------------ rowgroup_sum, colsum, transposes
@pytest.mark.parametrize("M,d,G_", S.ROWGROUP)
def test_rowgroup_families_and_mutant(M, d, G_):
    grp = S.make_groups(M, G_)
    assert 0 in grp.tolist() and G_ - 1 in grp.tolist() and int(((grp >= 0) & (grp < G_)).sum()) >= 1      # every case sums at least one row; the first and the last group are hit
    if M > 74:
        assert -1 in grp.tolist() and G_ in grp.tolist()
    if M > 512:
        assert 0 <= int(grp[511]) < G_ and grp[511] == grp[512]                                      # a run crosses the 512-row block seam
    x, f = S.ints(M, d, 5)
    o0 = S.ints_like((G_, d), f, 6)
    ref, A, n = S.rowgroup_ref(x, grp, o0)
    assert S.partial_sums_exact(A, f)
    ok = (grp >= 0) & (grp < G_)
    got = o0.to(F32).clone().index_add_(0, grp[ok], x.to(F32)[ok])
    assert S.mismatches(got, ref)[0] == 0
    xg, og = S.gauss((M, d), 7), S.gauss((G_, d), 8)
    refg, Ag, ng = S.rowgroup_ref(xg, grp, og)
    assert S.sum_ratio(og.clone().index_add_(0, grp[ok], xg[ok]), refg, Ag, ng) <= 1
    if M > 512:
        assert S.mismatches(S.rowgroup_ref(x, grp, o0, mutant="lose_seam_run")[0], ref)[0] > 0
        assert S.sum_ratio(S.rowgroup_ref(xg, grp, og, mutant="lose_seam_run")[0], refg, Ag, ng) > 1


@pytest.mark.parametrize("R,C", S.TRANSPOSE)
def test_colsum_transpose_and_mutants(R, C):
    x, f = S.ints(R, C, 9)
    c0 = S.ints_like((C,), f, 10)
    ref, A, n = S.colsum_ref(x, c0)
    assert S.partial_sums_exact(A, f) and torch.equal(x.to(BF16).double(), x)
    assert S.mismatches(c0.to(F32) + x.to(F32).sum(0), ref)[0] == 0 and S.mismatches(x.to(F32).flip(0).cumsum(0)[-1] + c0.to(F32), ref)[0] == 0
    assert S.mismatches(S.colsum_ref(x, c0, mutant="skip_last8")[0], ref)[0] > 0
    xg, cg = S.gauss((R, C), 11).to(BF16), S.gauss((C,), 12)
    refg, Ag, ng = S.colsum_ref(xg, cg)
    assert S.sum_ratio(cg + xg.float().sum(0), refg, Ag, ng) <= 1 and S.sum_ratio(S.colsum_ref(xg, cg, mutant="skip_last8")[0], refg, Ag, ng) > 1
    e = S.edges_bf16(R * C, 13).view(R, C)
    assert S.mismatches(S.transpose_ref(e), e.t())[0] == 0 and S.mismatches(S.transpose_ref(e, mutant="tile_rows_swapped"), e.t())[0] > 0


def test_cast_transpose_statement_and_padded_column_mutant():
    R, C = 67, 67
    w = S.edges(R * C, 14).view(R, C)
    o, ot = S.cast_transpose_ref(w)
    ok = ~torch.isnan(w)
    assert S.mismatches(o[ok], w.to(BF16)[ok])[0] == 0 and S.mismatches(ot, o.t())[0] == 0
    a = G.arena((R, C), C + 5, BF16, guard_rows=4)
    a.view.copy_(o)
    assert G.stray_count(a) == 0 and S.mismatches(a.view, o)[0] == 0
    a.buf.view(-1, C + 5)[4:4 + R, C] = o[:, 0]                                                      # a kernel that rounds C up to a whole 4-column group
    assert G.stray_count(a) == R


# ------------------------------------------------------------------------------------------------ timestep embedding
def test_timestep_reference_W_and_cap():
    w = {"schedule": 0.0, "far": 0.0}
    for dim in S.TIMESTEP_DIMS:
        for B in S.TIMESTEP_B:
            for fam, W in (("schedule", S.W_TIMESTEP), ("far", S.W_TIMESTEP_FAR)):
                sg = S.sigmas(B, fam, dim)
                ref, Sc = S.timestep_ref(sg, dim)
                f = S.timestep_f32(sg, dim)
                w[fam] = max(w[fam], S.measure_W(f, ref, Sc))
                E = S.timestep_E(Sc, W)
                assert not bool(S.outside(f.to(BF16), ref, E).any()) and S.worst_ratio(f.to(BF16), ref, E) <= 1
                if fam == "schedule":
                    assert float(sg.max()) <= 8 and S.ambiguous(ref, E) <= S.AMBIGUOUS_CAP, (dim, B, S.ambiguous(ref, E))
                    if B >= 4:
                        assert sg[:4].tolist() == [S.f32(v) for v in S.SIGMA_EDGE]
                else:
                    assert float(sg[0]) == 1000.0
                if dim % 2:
                    assert bool((ref[:, -1] == 0).all()) and bool((E[:, -1] == 0).all())           # the odd column is 0, exactly
    print(f"\nW timestep: measured {w['schedule']:.3f} (sigma <= 7), {w['far']:.3f} (sigma <= 1000); constants {S.W_TIMESTEP}, {S.W_TIMESTEP_FAR}")
    assert math.ceil(w["schedule"]) == S.W_TIMESTEP and math.ceil(w["far"]) == S.W_TIMESTEP_FAR
    assert abs(w["schedule"] - S.W_MEASURED["timestep"]) < 2e-2 and abs(w["far"] - S.W_MEASURED["timestep_far"]) < 2e-2


def test_timestep_mutants_rejected():
    for dim in (6, 7, 256):
        sg = S.sigmas(64, "schedule", dim)
        ref, Sc = S.timestep_ref(sg, dim)
        E = S.timestep_E(Sc)
        for m in ("cos_sin_swapped", "half_minus_1") + (("odd_tail_nonzero",) if dim % 2 else ()):
            mut = S.rne(S.timestep_ref(sg, dim, mutant=m)[0].to(F32))
            assert bool(S.outside(mut, ref, E).any()) and S.worst_ratio(mut, ref, E) > 1, (dim, m)
    sg = S.sigmas(64, "schedule", 2)
    ref, Sc = S.timestep_ref(sg, 2)
    assert bool(S.outside(S.rne(S.timestep_ref(sg, 2, mutant="cos_sin_swapped")[0].to(F32)), ref, S.timestep_E(Sc)).any())


# ------------------------------------------------------------------------------------------------ SiLU
def test_silu_reference_W_and_cap():
    x = S.all_finite_bf16()
    assert x.numel() == 65280
    xg = x.double().requires_grad_(True)
    y = torch.nn.functional.silu(xg)
    (g,) = torch.autograd.grad(y.sum(), xg)
    ref, Sc = S.silu_ref(x)
    big = ref.abs() >= S.MIN_NORMAL
    assert torch.allclose(ref[big], y.detach()[big], rtol=1e-13, atol=0)                             # the statement against torch's fp64 silu
    f = S.silu_f32(x)
    wf = S.measure_W(f, ref, Sc)
    E = S.silu_E(Sc)
    assert not bool(S.outside(f.to(BF16), ref, E).any()) and S.worst_ratio(f.to(BF16), ref, E) <= 1
    assert S.ambiguous(ref, E) <= S.AMBIGUOUS_CAP
    old = x.float() / (1 + torch.exp(-x.float()))                                                    # the formula without the branch below -80: -0 where the truth is ~1e-37
    assert bool(S.outside(old.to(BF16), ref, E)[x.float() < -88.8].any()) and not bool(S.outside(old.to(BF16), ref, E)[x.float() > -88].any())
    wb = 0.0
    for dy in S.silu_dys(x.numel()):
        rb, Sb = S.silu_bwd_ref(x, dy)
        assert torch.allclose(rb, dy.double() * g, rtol=1e-9, atol=1e-300)
        fb = S.silu_bwd_f32(x, dy)
        wb = max(wb, S.measure_W(fb, rb, Sb, S.SILU_BWD_FLOOR))
        Eb = S.silu_bwd_E(Sb)
        assert not bool(S.outside(fb.to(BF16), rb, Eb).any()) and S.worst_ratio(fb.to(BF16), rb, Eb) <= 1
        assert S.ambiguous(rb, Eb - S.SILU_BWD_FLOOR) <= S.AMBIGUOUS_CAP                              # the cap is held by the relative part; the floor concerns |ref| < 2^-91
        assert float((S.SILU_BWD_FLOOR > 2.0 ** -9 * rb.abs()).double().mean()) < 0.25 and bool((x.float()[S.SILU_BWD_FLOOR > 2.0 ** -9 * rb.abs()] < -60).all())
        mut = S.rne(S.silu_bwd_ref(x, dy, mutant="no_x_term")[0].to(F32))
        assert bool(S.outside(mut, rb, Eb).any()) and S.worst_ratio(mut, rb, Eb) > 1
    print(f"\nW silu_fwd: measured {wf:.3f}, constant {S.W_SILU_FWD};  W silu_bwd: measured {wb:.3f}, constant {S.W_SILU_BWD}")
    assert math.ceil(wf) == S.W_SILU_FWD and math.ceil(wb) == S.W_SILU_BWD
    assert abs(wf - S.W_MEASURED["silu_fwd"]) < 2e-2 and abs(wb - S.W_MEASURED["silu_bwd"]) < 2e-2


def test_achieved_is_the_interval():
    """achieved(got, ref) <= E exactly where got lies inside [rne(ref - E), rne(ref + E)] (up to the parity of a boundary that is itself a tie)"""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(20000, generator=g, dtype=F64) * torch.ldexp(torch.ones(20000, dtype=F64), torch.randint(-140, 20, (20000,), generator=g))
    got = S.round_bf16_64(ref * (1 + torch.randn(20000, generator=g, dtype=F64) * 2e-3)).to(BF16)
    E = ref.abs() * 2e-3
    out = S.outside(got, ref, E)
    a = S.achieved(got, ref)
    assert bool(out.any()) and bool((~out).any())
    assert bool((a[out] >= E[out]).all()) and bool((a[~out] <= E[~out]).all())
    assert S.achieved(torch.tensor([float("inf"), float("nan"), float("inf")]).to(BF16), torch.tensor([1e39, 1.0, 1.0], dtype=F64)).tolist() == [0.0, float("inf"), float("inf")]
