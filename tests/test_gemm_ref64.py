"""The reference of tests/test_gpu_gemm_exact.py on its own (CPU): for every (M, N, K) the GPU suite draws, the generator's exactness preconditions hold, three
fp32 emulations with different summation orders equal the fp64 reference element for element, enough results are exact bf16 rounding ties to tell
round-to-nearest-even from round-half-away, the fp32 column sums of the EPI_DGELU family are exact in two orders - and the comparator rejects three deliberately
broken emulations (a dropped K element of one row, round-half-away, one transposed 32 x 32 block)."""
import pytest
import torch

import gemm_ref64 as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SHAPES = R.all_mnk()


def _emulations(A, B):
    a, b = A.float(), B.float()
    K = a.shape[1]
    yield "plain", a @ b.t()
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=F32)
    for s in range(7):
        if s < K:
            acc += a[:, s::7] @ b[:, s::7].t()
    yield "7 strided K slices", acc
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=F32)
    for k0 in reversed(range(0, K, 64)):
        acc += a[:, k0:k0 + 64] @ b[:, k0:k0 + 64].t()
    yield "64-wide K tiles in reverse", acc


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_reference_conditions(M, N, K):
    """preconditions (the generator's assertions), three fp32 summation orders equal to fp64, and at least 1 % exact bf16 ties.  Sums of K < 32 products of
    magnitude <= 64 rarely need a ninth bit: there the bias family (a wider integer per element) carries the ties."""
    p = R.exact_operands(M, N, K, seed=M * 31 + N * 7 + K)
    for name, got in _emulations(p.A, p.B):
        n, where = R.mismatches(got, p.ref.to(F32))
        assert n == 0, f"{name}: {n} elements differ from fp64, first at {where}"
    assert torch.equal(R.rne_bf16(p.ref), p.ref.to(BF16))          # torch's cast of an fp64 tensor is the same round-to-nearest-even
    ref = p.ref if K >= 32 else R.exact_operands(M, N, K, seed=M * 31 + N * 7 + K, bias=True).ref_bias
    frac = float(R.is_bf16_tie(ref).double().mean())
    assert frac >= 0.01, f"only {frac:.4f} of the results are bf16 ties"


@pytest.mark.parametrize("M,N,K", R.NT_SMALL + R.NT_STAGGER + R.NT_PERSIST + [R.NT_PERSIST_320])
def test_bias_beta_and_dgelu_families(M, N, K):
    seed = M + N + K
    p = R.exact_operands(M, N, K, seed=seed, bias=True)            # asserts acc + bias exact
    got = (p.A.float() @ p.B.float().t()) + p.bias[None, :]
    assert R.mismatches(got, p.ref_bias.to(F32))[0] == 0
    c0, ref1 = R.exact_c0(p, seed=seed + 1)
    assert R.mismatches(c0 + p.A.float() @ p.B.float().t(), ref1.to(F32))[0] == 0
    q = R.exact_operands(M, N, K, seed=seed, row_scales="cols")
    for out_f32 in (True, False):
        aux, d0, c, db = R.exact_dgelu(q, seed=seed + 2, out_f32=out_f32)
        c32 = (q.A.float() @ q.B.float().t()) * aux.float()
        if not out_f32:
            c32 = c32.to(BF16).float()
        assert R.mismatches(c32, c.to(F32))[0] == 0
        fwd = d0 + c32.sum(0)                                      # torch's blocked sum
        back = c32.flip(0).cumsum(0)[-1] + d0                      # row by row, last row first, dbias0 last
        assert torch.equal(fwd.to(F64), db) and torch.equal(back.to(F64), db)


def test_gelu_reference():
    u = R.all_bf16_between(-100.0, 100.0)
    assert 34000 < u.numel() < 34400 and float(u[0]) == -100.0 and float(u[-1]) == 100.0
    x = u.double().requires_grad_(True)
    y = torch.nn.functional.gelu(x, approximate="tanh")
    (g,) = torch.autograd.grad(y.sum(), x)
    assert torch.allclose(R.gelu64(u), y.detach(), rtol=1e-12, atol=1e-14) and torch.allclose(R.dgelu64(u), g, rtol=1e-12, atol=1e-14)
    ey, eg = R.torch_gelu_excess()
    assert ey <= 0 and eg < 2.0 ** -20   # torch's fp32 gelu rounded to bf16 sits inside the bound the kernels are held to; its gelu' leaves it by < 1e-7 near the zero of gelu'
    p, uu = R.exact_gelu_operands(200, 136, 72, seed=3)
    assert float(uu.abs().max()) <= 8.5 and float(uu.abs().max()) > 4


def _half_away_bf16(x64):
    u = x64.to(F32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x8000) >> 16
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(BF16)


@pytest.mark.parametrize("M,N,K", [(333, 260, 128), (200, 136, 72)])
def test_comparator_rejects_broken_emulations(M, N, K):
    p = R.exact_operands(M, N, K, seed=5)
    a, b = p.A.float(), p.B.float()
    row = int((p.ia[:, K - 1] != 0).nonzero()[-1])
    a_drop = a.clone()
    a_drop[row, K - 1] = 0.0                                       # the last K element of one row not counted
    n, where = R.mismatches(a_drop @ b.t(), p.ref.to(F32))
    assert n > 0 and all(r == row for r, _ in where)
    n, _ = R.mismatches(_half_away_bf16(p.ref), R.rne_bf16(p.ref))   # round-half-away in the bf16 store
    assert n > 0
    swapped = (a @ b.t()).clone()
    swapped[64:96, 32:64] = swapped[64:96, 32:64].t().clone()      # one 32 x 32 fragment stored transposed
    n, where = R.mismatches(swapped, p.ref.to(F32))
    assert n > 0 and all(64 <= r < 96 and 32 <= c < 64 for r, c in where)
    assert R.mismatches(a @ b.t(), p.ref.to(F32))[0] == 0 and R.mismatches((a @ b.t()).to(BF16), R.rne_bf16(p.ref))[0] == 0


def test_arena_detects_stray_writes():
    for dtype in (BF16, F32):
        a = R.arena((5, 12), 16, dtype, guard_rows=3, fill=torch.ones(5, 12))
        assert torch.isnan(a.buf.float()).sum() == a.buf.numel() - 60 and a.view.data_ptr() % 16 == 0
        R.assert_untouched(a)
        a.view.fill_(2.0)
        R.assert_untouched(a)
        a.buf[3 * 16 + 12] = 0.0                                   # a pad column of the first row
        assert R.stray_count(a) == 1
        a.poison()
        assert torch.isnan(a.view.float()).all()
