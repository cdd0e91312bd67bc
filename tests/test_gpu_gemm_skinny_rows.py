"""udm_gemm_skinny_bf16 at 65 .. 128 rows (csrc/decode.hip: two row groups in one workgroup, rows [0, 64) and [64, M), on the same weight fragments).

1. Exact against fp64.  Operands of tests/gemm_ref64.exact_operands: every fp32 partial sum is exact, so any summation order gives the reference - an fp32
   output EQUALS the fp64 product, a bf16 output its round-to-nearest-even, through the bias as well; the GELU epilogue is held per element to
   2^-8 |ref| + 2^-20 (plus twice what torch's own fp32 evaluation exceeds it by, where it does: the rule of tests/test_gpu_gemm_exact.py).  Operands and
   outputs are views in NaN arenas with padded leading dimensions, the K-split workspace is NaN before every call, and every element outside the M x N output
   is compared bit for bit.
2. Bit-equality with the row halves.  Gaussian operands, so the order matters: with one workspace large enough for all three calls (the K split is then
   the same) out[:64] is torch.equal to the call on a[:64] - the kernel that serves up to 64 rows - and out[64:] to the call on a[64:M]; every epilogue, both
   output types, and the vocabulary head of UniDisc-S (N = 40193, not a multiple of 32).
3. M = 129 is refused with a message naming 128 and nothing is written."""
import functools
import math

import pytest
import torch

import gemm_ref64 as R

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
NAN = float("nan")
ROWS = (65, 72, 80, 127, 128)


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def up(n, m):
    return (n + m - 1) // m * m


@functools.lru_cache(maxsize=8)
def problem(M, N, Kd, family):
    """the drawn problem of a shape, shared by its cases and never modified: 'plain' | 'bias' | 'gelu'"""
    seed = M * 31 + N * 7 + Kd
    if family == "gelu":
        return R.exact_gelu_operands(M, N, Kd, seed=seed)
    return R.exact_operands(M, N, Kd, seed=seed, bias=(family == "bias"))


def place(x, *, pad=8, mult=8):
    rows, cols = x.shape
    return R.arena((rows, cols), up(cols, mult) + pad, x.dtype, device=DEV, fill=x)


def blank(rows, cols, dtype):
    mult = 8 if dtype == BF16 else 4
    return R.arena((rows, cols), up(cols, mult) + mult, dtype, device=DEV)


@functools.lru_cache(maxsize=1)
def gelu_allowance():
    return max(0.0, 2 * R.torch_gelu_excess()[0])


@pytest.mark.parametrize("N,Kd", R.SKINNY_NK)
@pytest.mark.parametrize("M", ROWS)
def test_exact_against_fp64(K, M, N, Kd):
    faults = []
    need = K.skinny_ws_elems(M, N, Kd)
    assert (need > 0) == (Kd >= 768)                       # K = 64: no split; K = 768, 3072: split through the workspace
    ws = torch.empty(max(need, 16), dtype=F32, device=DEV)
    for epi in ("none", "bias", "gelu"):
        for cd in (BF16, F32):
            what = f"{epi} {'f32' if cd == F32 else 'bf16'}"
            ws.fill_(NAN)
            if epi == "gelu":
                p, u = problem(M, N, Kd, "gelu")
            else:
                p = problem(M, N, Kd, "plain" if epi == "none" else "bias")
            a, w, c = place(p.A), place(p.B), blank(M, N, cd)
            arenas = [a, w, c]
            kw = {}
            if epi != "none":
                bias = place(p.bias[None, :], mult=4, pad=4)
                arenas.append(bias)
                kw = dict(epilogue=K.EPI_BIAS if epi == "bias" else K.EPI_BIAS_GELU, bias=bias.view[0])
            K.gemm_skinny(a.view, w.view, out=c.view, ws=ws, **kw)
            torch.cuda.synchronize()
            if epi == "gelu":
                ref = R.gelu64(u).to(DEV)
                ex = R.gelu_excess(c.view, ref) if bool(torch.isfinite(c.view.float()).all()) else float("inf")
                if ex > gelu_allowance():
                    faults.append(f"{what}: excess {ex:.3e} over 2^-8 |ref| + 2^-20 (allowed {gelu_allowance():.3e})")
            else:
                ref = p.ref if epi == "none" else p.ref_bias
                n, where = R.mismatches(c.view, ref if cd == F32 else R.rne_bf16(ref))
                if n:
                    faults.append(f"{what}: {n} of {M * N} elements differ from the reference, first (row, col) {where}")
            stray = sum(R.stray_count(x) for x in arenas)
            if stray:
                faults.append(f"{what}: {stray} arena elements outside the output changed")
            if need and not bool(torch.isfinite(ws[:2 * M * N]).all()):
                faults.append(f"{what}: the first two K slabs of the workspace were not all written")
            if not need and bool(torch.isfinite(ws).any()):
                faults.append(f"{what}: the workspace was written by a call that must not split")
    assert not faults, f"skinny {M}x{N}x{Kd}:\n  " + "\n  ".join(faults)


def _gauss(M, N, Kd, seed):
    gen = torch.Generator().manual_seed(seed)
    Np = up(N, 128)                                        # (the head's weight shadow has padded rows, its logits buffer a padded row stride)
    a = torch.randn(M, Kd, generator=gen).to(BF16).to(DEV)
    w = (torch.randn(Np, Kd, generator=gen) / math.sqrt(Kd)).to(BF16).to(DEV)
    bias = (torch.randn(N, generator=gen) * 0.5).to(DEV)
    return a, w, bias, Np


def _halves_case(K, M, N, Kd, epis):
    a, w, bias, Np = _gauss(M, N, Kd, M + 3 * N + Kd)
    ws = torch.empty(max(K.skinny_ws_elems(M, N, Kd), 16), dtype=F32, device=DEV)      # holds the split of M rows, so of 64 and of M - 64 too
    for epi in epis:
        for cd in (BF16, F32):
            kw = dict(N=N, ws=ws, epilogue=epi, bias=bias if epi != K.EPI_NONE else None)
            out = torch.full((M, Np), NAN, dtype=cd, device=DEV)
            lo = torch.full((64, Np), NAN, dtype=cd, device=DEV)
            hi = torch.full((M - 64, Np), NAN, dtype=cd, device=DEV)
            ws.fill_(NAN)
            K.gemm_skinny(a, w, out=out, **kw)
            ws.fill_(NAN)
            K.gemm_skinny(a[:64], w, out=lo, **kw)
            ws.fill_(NAN)
            K.gemm_skinny(a[64:], w, out=hi, **kw)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out[:, :N].float()).all()), (M, N, Kd, epi, cd)
            assert torch.equal(out[:64, :N], lo[:, :N]), (M, N, Kd, epi, cd, "rows [0, 64)")
            assert torch.equal(out[64:, :N], hi[:, :N]), (M, N, Kd, epi, cd, "rows [64, M)")
            assert bool(torch.isnan(out[:, N:].float()).all())                           # nothing past N is written
            ref = a.float() @ w[:N].float().t()                                          # (and the halves are the product, not merely each other)
            if epi == K.EPI_NONE:
                assert float((out[:, :N].float() - ref).abs().max()) < 0.1


@pytest.mark.parametrize("N,Kd", R.SKINNY_NK)
@pytest.mark.parametrize("M", ROWS)
def test_rows_equal_the_64_row_kernel_on_the_halves(K, M, N, Kd):
    _halves_case(K, M, N, Kd, (K.EPI_NONE, K.EPI_BIAS, K.EPI_BIAS_GELU))


@pytest.mark.parametrize("M", (65, 128))
def test_rows_equal_the_halves_at_the_vocabulary_head(K, M):
    _halves_case(K, M, 40193, 768, (K.EPI_BIAS,))


def test_129_rows_are_refused_and_nothing_is_written(K):
    a, w, _, Np = _gauss(129, 192, 64, 1)
    out = torch.full((129, Np), NAN, dtype=BF16, device=DEV)
    ws = torch.full((1 << 16,), NAN, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="128"):
        K.gemm_skinny(a, w, out=out, N=192, ws=ws)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(ws).all())
    assert K.SKINNY_MAX_ROWS == 128
