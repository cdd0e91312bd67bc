"""The comparator of tests/engine_gemm_audit.py on the CPU: fp32 emulations of the kernels' arithmetic stay inside every bound, one training step of the engine on
the CPU doubles (tests/fake_kernels.py) passes the audit, and every mutant - a one-line wrapper around a double - is rejected with a message naming the call."""
import pytest
import torch

import engine_gemm_audit as E
import fake_kernels
import gemm_ref64 as R
import ledger

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TEST = "engine_gemm_audit_host"
# (M, N, K) of the engine's calls in tests/test_gpu_engine_gemm_audit.py (d = 256, 1024 rows: qkv, out-proj, mlp.0, mlp.2, their weight gradients, the split head on
# 192 compacted rows) and one long contraction
SHAPES = [(1024, 768, 256), (1024, 256, 256), (1024, 1024, 256), (1024, 256, 1024), (768, 256, 1024), (256, 1024, 1024), (192, 1513, 256), (256, 256, 24576)]


@pytest.fixture()
def fake_k(monkeypatch):
    import unidisc_amd.dit as dit_mod
    import unidisc_amd.diffusion as diff_mod

    monkeypatch.setattr(dit_mod, "K", fake_kernels)
    monkeypatch.setattr(diff_mod, "K", fake_kernels)
    return fake_kernels


def _operands(M, N, Kd, family, seed):
    gen = torch.Generator().manual_seed(seed)
    A, B = torch.randn(M, Kd, generator=gen), torch.randn(N, Kd, generator=gen)
    if family == "positive":   # no cancellation: |ref| = S, the worst case of the bound
        A, B = A.abs(), B.abs()
    return A.to(BF16), B.to(BF16)


def _emulations(A, B):
    """fp32 accumulators of A B^T: one matmul, and 8 K slices summed in reverse order (a split-K reduce)"""
    a, b = A.float(), B.float()
    whole = a @ b.t()
    step = A.shape[1] // 8
    parts = [a[:, i * step:(i + 1) * step] @ b[:, i * step:(i + 1) * step].t() for i in range(8)]
    sliced = parts[-1].clone()
    for p in reversed(parts[:-1]):
        sliced += p
    return whole, sliced


# ------------------------------------------------------------------------------------------------ reference emulations
@pytest.mark.parametrize("family", ["randn", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulations_stay_inside_the_bounds(shape, family):
    M, N, Kd = shape
    A, B = _operands(M, N, Kd, family, seed=M + N + Kd)
    A64, B64 = A.to(F64), B.to(F64)
    whole, sliced = _emulations(A, B)
    for what, acc in (("whole", whole), ("8 slices reversed", sliced)):
        ledger.check(TEST, f"{shape} {family} {what} fp32", E.check_product(acc, A64, B64), 1.0)
        ledger.check(TEST, f"{shape} {family} {what} bf16", E.check_product(acc.to(BF16), A64, B64), 1.0)
    ref, S, n, exact = E.product_ref(A64, B64)
    assert not exact
    a = E.acc_bound(S, n)
    ledger.check(TEST, f"{shape} {family} two orders fp32 / 2 x bound", E.worst_ratio((whole.to(F64) - sliced.to(F64)).abs(), 2 * a), 1.0)
    ledger.check(TEST, f"{shape} {family} two orders bf16 / 2 x bound",
                 E.worst_ratio((whole.to(BF16).to(F64) - sliced.to(BF16).to(F64)).abs(), 2 * E.bf16_bound(ref, a)), 1.0)


@pytest.mark.parametrize("family", ["randn", "positive"])
def test_fp32_emulations_of_the_epilogues_stay_inside_the_bounds(family):
    M, N, Kd = 1024, 1024, 256        # mlp.0 forward; the mlp.2 dgrad has the same extents with K = 256 as its contraction
    A, B = _operands(M, N, Kd, family, seed=9)
    A, B = (A.float() * 0.25).to(BF16), (B.float() * 0.25).to(BF16)      # pre-activations of a few units
    A64, B64 = A.to(F64), B.to(F64)
    gen = torch.Generator().manual_seed(10)
    bias, prior = torch.randn(N, generator=gen), torch.randn(M, N, generator=gen)
    for what, acc in zip(("whole", "8 slices reversed"), _emulations(A, B)):
        ledger.check(TEST, f"{family} {what} bias bf16", E.check_product((acc + bias).to(BF16), A64, B64, bias=bias.to(F64)), 1.0)
        ledger.check(TEST, f"{family} {what} beta=1 fp32", E.check_product(acc + prior, A64, B64, prior=prior.to(F64), beta=1.0), 1.0)
        u = (acc + bias).to(BF16).float()
        c, aux = torch.nn.functional.gelu(u, approximate="tanh").to(BF16), E.dgelu_formula_f32(u).to(BF16)
        rc, ra = E.check_gelu(c, aux, A64, B64, bias.to(F64))
        ledger.check(TEST, f"{family} {what} bias_gelu C", rc, 1.0)
        ledger.check(TEST, f"{family} {what} bias_gelu aux", ra, 1.0)
        d0 = torch.randn(N, generator=gen)
        dc = (acc * aux.float()).to(BF16)
        rc, rs = E.check_dgelu(dc, A64, B64, aux.to(F64), d0.to(F64), d0 + dc.float().sum(0))
        ledger.check(TEST, f"{family} {what} dgelu C", rc, 1.0)
        ledger.check(TEST, f"{family} {what} dgelu column sums", rs, 1.0)
        # the comparator can fail: the column sums of the unrounded products are not those of the stored values; a pre-activation one bf16 step off is no candidate
        assert E.check_dgelu(dc, A64, B64, aux.to(F64), d0.to(F64), d0 + (acc * aux.float()).sum(0))[1] > 1.0
        off = E._bf16_succ(E._bf16_succ(u.to(BF16))).float()
        assert max(E.check_gelu(torch.nn.functional.gelu(off, approximate="tanh").to(BF16), E.dgelu_formula_f32(off).to(BF16), A64, B64, bias.to(F64))) > 1.0


def test_the_gelu_derivative_formula_term_is_the_documented_one():
    term = E.dgelu_formula_term()
    ledger.record(TEST, "fp32 gelu' formula of gelu_tanh_both vs dgelu64, every bf16 in [-12, 12]: 2 x worst |error|", term)
    assert abs(term - 2.95e-07) < 0.01e-07, term                     # the number in the docstring of tests/engine_gemm_audit.py
    assert term < 2.0 ** -20                                          # far below the cancellation term of gelu_bound, let alone the bf16 rounding


def test_no_row_split_fires_at_the_audited_shapes_with_16_cus_held(monkeypatch):
    """why tests/test_gpu_engine_gemm_audit.py has no held-CUs case: at d = 256 and 1024 rows every GEMM has at most 16 tiles, so `_row_split` (which cuts a single
    round of MORE tiles than the CUs left) never fires under gemm_set_cus(16)"""
    from unidisc_amd import kernels as K

    monkeypatch.setattr(K, "_CUS", [16])
    for rows, cols in ((1024, 768), (1024, 256), (1024, 1024)):     # gemm_nt / gemm_nn: forward and dgrad outputs
        assert K._row_split(rows, cols, (320, 256, 192)) is None, (rows, cols)
    for out, inp in ((768, 256), (256, 256), (1024, 256), (256, 1024)):   # gemm_tn: the block weight gradients
        assert K._row_split(out, inp, (256, 192)) is None, (out, inp)
    assert K._row_split(1024, 1536, (320, 256, 192)) == 512          # (the rule itself is alive: 24 tiles over 16 CUs)


# ------------------------------------------------------------------------------------------------ the engine on the CPU doubles
@pytest.mark.parametrize("model", ["plain", "plain_adaln", "mm"])
def test_one_fake_kernel_training_step_passes_the_audit(model, fake_k, monkeypatch):
    diff = E.build(model, "cpu")
    bb = diff.backbone
    with E.audit(monkeypatch, fake_kernels, f"{TEST} {model}") as aud:
        E.step(diff, E.batch(model, 2))
        calls = aud.resolve(bb)
        gaps = aud.padding_gaps()
    assert all(torch.isfinite(p.grad).all() for p in bb.parameters() if p.grad is not None)
    assert all(float(g.abs().max()) == 0.0 for g in gaps if g.numel())
    names = {c.name for c in calls}
    assert {"gemm_nt", "gemm_tn_splitk", "gemm_nt_splitk"} <= names, names     # (gemm_nn: the dgrad-from-W regime exists on the GPU only)
    assert ("small_batch_linear_bwd" in names) == (model == "plain_adaln")
    assert all(r <= 1.0 for c in calls for r in c.ratios.values()) and all(c.ratios for c in calls)
    # the outermost call is audited, the double's inner gemm_nt of gemm_nt_splitk is not counted again
    assert all(c.inner == ["gemm_nt"] for c in calls if c.name == "gemm_nt_splitk")
    # every GEMM weight's gradient was written by an audited call, and its operands were kept
    for ln, lin in bb._lins.items():
        name = next(n for n, p in bb.named_parameters() if p is lin.weight)
        assert aud.by(grad=name) and (aud.operands.get(name) or aud.by(name="small_batch_linear_bwd", grad=name)), name
    # forward GEMMs read w16, the dgrads the transposed shadow: every block Linear is read in both forms
    for ln in (f"{i}.{k}" for i in range(2) for k in ("qkv", "out", "fc1", "fc2")):
        assert aud.by(name="gemm_nt", weight=(ln, "w16")) and aud.by(name="gemm_nt", weight=(ln, "w16t")), ln
    if model == "mm":   # two head groups in the forward, the second on the weight rows from the aligned boundary below the text vocabulary
        assert sorted(c.c0 for c in aud.by(name="gemm_nt", weight=("head", "w16"))) == [0, bb._head_split_cols()[0]]


# ------------------------------------------------------------------------------------------------ mutants
def _rejected(monkeypatch, mutants, naming, model="plain", direct=None):
    """install the mutants over the doubles, run a step (or `direct`) under the auditor, and return the failure, which must name the call"""
    for name, make in mutants.items():
        monkeypatch.setattr(fake_kernels, name, make(getattr(fake_kernels, name)))
    with pytest.raises(AssertionError, match=naming) as ei:
        with E.audit(monkeypatch, fake_kernels, TEST + " mutant", record=False):
            if direct is not None:
                direct()
            else:
                E.step(E.build(model, "cpu"), E.batch(model, 2))
    return str(ei.value)


def test_mutant_contraction_short_of_its_last_64_rows_is_rejected(fake_k, monkeypatch):
    m = lambda real: lambda a, b, out, **kw: real(a[:-64], b[:-64], out, **kw)
    _rejected(monkeypatch, dict(gemm_tn=m, gemm_tn_splitk=m), r"gemm_tn_splitk \(768, 256, 256\)")


def test_mutant_unwritten_output_tile_is_rejected_through_the_poisoned_gradients(fake_k, monkeypatch):
    def m(real):
        def tn(a, b, out, **kw):
            keep = out[:256, :256].clone()
            real(a, b, out, **kw).__setitem__((slice(0, 256), slice(0, 256)), keep)
            return out
        return tn
    msg = _rejected(monkeypatch, dict(gemm_tn=m, gemm_tn_splitk=m), r"gemm_tn_splitk \(768, 256, 256\)")
    assert "inf" in msg          # a NaN, not a near miss


def test_mutant_weight_in_place_of_its_transpose_is_rejected(fake_k, monkeypatch):
    m = lambda real: lambda a, b, *r, **kw: real(a, b.t().contiguous() if b.shape[0] == b.shape[1] else b, *r, **kw)
    _rejected(monkeypatch, dict(gemm_nt=m), r"gemm_nt \(256, 256, 256\)")


def _half_away(x32):
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = ((u + 0x8000) >> 16) & 0xFFFF
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(BF16)


def test_mutant_rounding_half_away_from_zero_is_rejected(fake_k, monkeypatch):
    p = R.exact_operands(64, 64, 64, seed=3, row_scales=False)       # integer operands: the fp32 accumulator is exact, ties among the results
    assert int(R.is_bf16_tie(p.ref).sum()) > 0
    call = lambda: fake_kernels.gemm_nt(p.A, p.B)
    with E.audit(monkeypatch, fake_kernels, TEST + " exact", record=False):
        call()                                                       # round-to-nearest-even passes
    m = lambda real: lambda a, b, **kw: _half_away(real(a, b, out_dtype=F32, **kw))
    _rejected(monkeypatch, dict(gemm_nt=m), r"gemm_nt \(64, 64, 64\)", direct=call)


def test_mutant_that_skips_the_beta_prior_is_rejected(fake_k, monkeypatch):
    A, B = _operands(256, 256, 128, "randn", seed=4)
    call = lambda: fake_kernels.gemm_tn(A.t().contiguous(), B.t().contiguous(), torch.randn(256, 256, generator=torch.Generator().manual_seed(5)), beta=1.0)
    with E.audit(monkeypatch, fake_kernels, TEST + " beta", record=False):
        call()
    m = lambda real: lambda a, b, out, **kw: real(a, b, out, **dict(kw, beta=0.0))
    _rejected(monkeypatch, dict(gemm_tn=m), r"gemm_tn \(256, 256, 128\) epi=none beta=1", direct=call)


def test_mutant_column_sums_of_the_wrong_matrix_are_rejected(fake_k, monkeypatch):
    def m(real):
        def nt(a, b, out=None, **kw):
            if kw.get("epilogue") != fake_kernels.EPI_DGELU:
                return real(a, b, out, **kw)
            return real(a, b, out, **dict(kw, bias=None)), kw["bias"].add_(kw["aux"].float().sum(0))
        return lambda *a, **kw: (lambda r: r[0] if isinstance(r, tuple) else r)(nt(*a, **kw))
    msg = _rejected(monkeypatch, dict(gemm_nt=m), r"gemm_nt \(256, 1024, 256\) epi=dgelu beta=0 column sums")
    assert "epi=dgelu beta=0 C:" not in msg                          # the product itself is right
