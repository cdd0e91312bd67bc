"""Operands whose GEMM is exact in fp32, their fp64 reference, and NaN arenas - the helpers of tests/test_gemm_ref64.py (CPU) and tests/test_gpu_gemm_exact.py.

bf16 x bf16 products are exact in fp32.  With A[i, k] = a_ik 2^(e_i) and B[j, k] = b_jk 2^(f_j), a, b integers in [-8, 8], every partial sum of
sum_k A[i, k] B[j, k] over ANY subset of k is an integer of magnitude <= 64 K times the power of two 2^(e_i + f_j): exactly representable in fp32 while
64 K < 2^24.  An fp32 accumulator therefore holds the exact result whatever the order, the split of K, a workspace or atomics in between, so an fp32 output
equals the fp64 reference and a bf16 output its round-to-nearest-even rounding - element by element, with no tolerance to choose.

Companions keep that property through the epilogues:
  bias     t_j 2^(f_j - r), t integer in [-8, 8], r the half-width of the scale range (so a multiple of 2^(e_min + f_min)); acc + bias is an integer below
           2^24 times 2^(e_min + f_j).  The scale range is narrowed from 6 until that holds for the drawn integers (`exact_operands(..., bias=True)`).
  C0       c_ij 2^(e_i + f_j) (beta = 1): every partial sum of C0 + acc stays an integer below 2^24 in the element's own scale.
  aux      one of {0, +-0.5, +-1, +-2} (EPI_DGELU): acc * aux is a half-integer; with e_i = 0 a column shares the scale 2^(f_j - 1), the sum of the |terms| of a
           column stays below 2^24 of those units, so the fp32 column sums (atomics, any order) are exact too - of the fp32 values, or of the bf16-rounded ones.
Comparisons are by value (`!=`): a NaN never compares equal, +0 and -0 do."""
import functools
import types

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LIMIT = 1 << 24
AUX_SET = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
NAN_BITS = {BF16: 0x7FA5, F32: 0x7FC5A5A5}      # quiet NaNs with a recognisable payload
INT_VIEW = {BF16: torch.int16, F32: torch.int32}
GUARD_ROWS = 384                                # more than the tallest tile (320 rows): a whole tile read or written behind the last row lands here


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _ints(shape, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


def _bf16_exact(x64, what):
    y = x64.to(BF16)
    assert torch.equal(y.to(F64), x64), f"{what}: not exactly representable in bf16"
    return y


def _f32_exact(x64, what):
    y = x64.to(F32)
    assert torch.equal(y.to(F64), x64), f"{what}: not exactly representable in fp32"
    return y


def rne_bf16(x64):
    """fp64 -> bf16 by round-to-nearest-even, written out on the bits (independent of torch's cast; tests/test_gemm_ref64.py compares the two).
    Exact for values that are fp32-representable (every reference here is); returns a bf16 tensor."""
    x32 = _f32_exact(x64, "rne_bf16 input")
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    u = torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)
    return u.view(BF16)


def is_bf16_tie(x64):
    """exactly half-way between two neighbouring bf16 values"""
    u = _f32_exact(x64, "tie input").contiguous().view(torch.int32).to(torch.int64) & 0xFFFF
    return u == 0x8000


_C0 = 0.7978845608028654      # sqrt(2 / pi)
_C1 = 0.044715


def gelu64(u):
    u = u.to(F64)
    return 0.5 * u * (1.0 + torch.tanh(_C0 * (u + _C1 * u ** 3)))


def dgelu64(u):
    u = u.to(F64)
    t = torch.tanh(_C0 * (u + _C1 * u ** 3))
    return 0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * _C0 * (1.0 + 3.0 * _C1 * u * u)


def gelu_bound(ref64):
    """|got - ref| <= 2^-8 |ref| + 2^-20: 2^-9 for the final bf16 rounding, 2^-9 for the fp32 evaluation in front of a rounding, 2^-20 for the cancellation
    at the zero of gelu' (about 16 fp32 roundings on terms of size 1)."""
    return 2.0 ** -8 * ref64.abs() + 2.0 ** -20


def gelu_excess(got, ref64):
    """largest (|got - ref| - bound) over the elements: <= 0 when the bound holds everywhere"""
    return float(((got.to(F64) - ref64).abs() - gelu_bound(ref64)).max())


def gelu_ratio(got, ref64):
    """largest |got - ref| / bound over the elements: <= 1 when the bound holds everywhere"""
    return float(((got.to(F64) - ref64).abs() / gelu_bound(ref64)).max())


@functools.lru_cache(maxsize=4)
def torch_gelu_excess(lo=-100.0, hi=100.0):
    """the same excess for torch's own fp32 gelu(approximate='tanh') and its autograd derivative, rounded to bf16, over every bf16 value in [lo, hi]:
    (excess of gelu, excess of gelu')"""
    u = all_bf16_between(lo, hi).float().requires_grad_(True)
    y = torch.nn.functional.gelu(u, approximate="tanh")
    (g,) = torch.autograd.grad(y.sum(), u)
    u64 = u.detach().to(F64)
    return gelu_excess(y.detach().to(BF16), gelu64(u64)), gelu_excess(g.to(BF16), dgelu64(u64))


def all_bf16_between(lo, hi):
    """every finite bf16 value in [lo, hi] (both zeros once), ascending"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF16)
    f = v.float()
    keep = torch.isfinite(f) & (f >= lo) & (f <= hi) & (bits != torch.tensor(-0x8000, dtype=torch.int16))
    return v[keep][torch.argsort(f[keep])]


def exact_operands(M, N, K, *, seed, row_scales=True, bias=False, scale_half_width=6):
    """A [M, K], B [N, K] bf16 and the fp64 reference A B^T of a problem whose every fp32 partial sum is exact.

    row_scales: True - e_i and f_j drawn from [-r, r]; "cols" - e_i = 0, f_j drawn (the EPI_DGELU family: a column shares one scale); False - no scales.
    bias: also draw a bias and narrow r until acc + bias is exact (see the module docstring).
    Returns a namespace: A, B, ref (fp64 [M, N]), ia, ib (the integers), e, f, r, smax, bias (fp32 [N] or None), ref_bias (fp64)."""
    gen = _gen(seed)
    assert 64 * K < LIMIT, "K too long: a partial sum could leave the 24-bit integers"
    ia, ib = _ints((M, K), gen), _ints((N, K), gen)
    S = ia.to(F64) @ ib.to(F64).t() + 0.0                       # integers below 2^53: exact
    smax = int(S.abs().max())
    sabs = int((ia.abs().to(F64) @ ib.abs().to(F64).t()).max()) if M * N * K <= (1 << 28) else 64 * K   # bound of every partial sum of every order
    assert smax <= sabs < LIMIT
    r = scale_half_width if row_scales else 0
    t = _ints((N,), gen)
    if bias:
        while r > 0 and smax * 2 ** (2 * r) + 8 >= LIMIT:
            r -= 1
        assert smax * 2 ** (2 * r) + 8 < LIMIT, "acc + bias would not be exact"
    e = _ints((M,), gen, -r, r) if row_scales is True else torch.zeros(M, dtype=torch.int64)
    f = _ints((N,), gen, -r, r) if row_scales else torch.zeros(N, dtype=torch.int64)
    A = _bf16_exact(torch.ldexp(ia.to(F64), e[:, None]), "A")
    B = _bf16_exact(torch.ldexp(ib.to(F64), f[:, None]), "B")
    ref = torch.ldexp(S, (e[:, None] + f[None, :]))
    _f32_exact(ref, "reference")
    out = types.SimpleNamespace(M=M, N=N, K=K, A=A, B=B, ref=ref, e=e, f=f, r=r, smax=smax, sabs=sabs, bias=None, ref_bias=None, ia=ia, ib=ib)
    if bias:
        b64 = torch.ldexp(t.to(F64), f - r)
        out.bias = _f32_exact(b64, "bias")
        out.ref_bias = ref + b64[None, :]
        _f32_exact(out.ref_bias, "acc + bias")
    return out


def exact_c0(p, *, seed):
    """C0 for beta = 1: c_ij 2^(e_i + f_j), c integer in [-8, 8]; returns (C0 fp32, fp64 reference C0 + A B^T)"""
    c = _ints((p.M, p.N), _gen(seed))
    assert p.sabs + 8 < LIMIT
    c0 = torch.ldexp(c.to(F64), p.e[:, None] + p.f[None, :])
    return _f32_exact(c0, "C0"), _f32_exact(c0 + p.ref, "C0 + acc").to(F64)


def exact_dgelu(p, *, seed, out_f32):
    """EPI_DGELU on a problem drawn with row_scales='cols': aux from AUX_SET, dbias0 integer-valued in the column's scale.
    Returns (aux bf16 [M, N], dbias0 fp32 [N], C reference fp64 (rounded to bf16 values unless out_f32), dbias reference fp64 [N])."""
    assert int(p.e.abs().max()) == 0, "the EPI_DGELU family needs e_i = 0 (row_scales='cols')"
    gen = _gen(seed)
    aux64 = torch.tensor(AUX_SET, dtype=F64)[torch.randint(0, len(AUX_SET), (p.M, p.N), generator=gen)]
    c = p.ref * aux64
    _f32_exact(c, "acc * aux")
    if not out_f32:
        c = rne_bf16(c).to(F64)
    d0 = torch.ldexp(_ints((p.N,), gen).to(F64), p.f)
    unit = torch.ldexp(torch.ones(p.N, dtype=F64), p.f - 1)      # every term of column j is an integer multiple of 2^(f_j - 1) (rounding to bf16 keeps that)
    assert torch.equal(torch.round(c / unit), c / unit)
    assert float(((c.abs().sum(0) + d0.abs()) / unit).max()) < LIMIT, "a column sum could leave the 24-bit integers"
    db = d0 + c.sum(0)
    _f32_exact(db, "dbias")
    return _bf16_exact(aux64, "aux"), _f32_exact(d0, "dbias0"), c, db


def exact_gelu_operands(M, N, K, *, seed):
    """EPI_BIAS_GELU, random family: exact operands scaled by one power of two so that u = bf16(acc + bias) spans about [-8, 8].
    Returns (problem with bias, u as fp64)."""
    p = exact_operands(M, N, K, seed=seed, row_scales=False, bias=True)
    g = 0
    while p.smax * 2.0 ** -g > 8.0:
        g += 1
    ha, hb = g // 2, g - g // 2
    p.A = _bf16_exact(torch.ldexp(p.A.to(F64), torch.tensor(-ha)), "A")
    p.B = _bf16_exact(torch.ldexp(p.B.to(F64), torch.tensor(-hb)), "B")
    p.ref = torch.ldexp(p.ref, torch.tensor(-g))
    p.bias = _f32_exact(torch.ldexp(p.bias.to(F64), torch.tensor(-g)), "bias")
    p.ref_bias = _f32_exact(p.ref + p.bias.to(F64)[None, :], "acc + bias").to(F64)
    return p, rne_bf16(p.ref_bias).to(F64)


def tn_layout(x):
    """[rows, K] operand -> its K-major [K, rows] layout (gemm_tn reads A[K, M], B[K, N])"""
    return x.t().contiguous()


def nn_layout(b):
    """B [N, K] -> [K, N] (gemm_nn computes a[M, K] @ b[K, N])"""
    return b.t().contiguous()


# ------------------------------------------------------------------------------------------------ NaN arenas
class Arena:
    """A [rows, cols] view with row stride `ld` in the middle of one larger allocation filled with a NaN of known payload: `guard_rows` rows of `ld`
    elements before and after it, and the pad columns [cols, ld) of every row.  A read past the view meets NaN, a write past it changes known bits."""

    def __init__(self, shape, ld, dtype, guard_rows=GUARD_ROWS, device="cpu", col0=0):
        rows, cols = shape
        assert ld >= col0 + cols
        self.dtype, self.ld, self.rows, self.cols, self.guard, self.col0 = dtype, ld, rows, cols, guard_rows, col0
        n = (rows + 2 * guard_rows) * ld
        self.bits = NAN_BITS[dtype]
        self.raw = torch.full((n,), self.bits, dtype=INT_VIEW[dtype], device=device)
        self.buf = self.raw.view(dtype)
        self.view = self.buf[guard_rows * ld:(guard_rows + rows) * ld].view(rows, ld)[:, col0:col0 + cols]

    def poison(self):
        """refill the view itself with the NaN (an output that must be overwritten, never read)"""
        self.view.copy_(torch.full((1,), self.bits, dtype=INT_VIEW[self.dtype], device=self.raw.device).view(self.dtype).expand(self.rows, self.cols))
        return self


def arena(shape, ld, dtype, guard_rows=GUARD_ROWS, device="cpu", fill=None, col0=0):
    """col0: the view starts at this column of the rows (an output that is a column slice of a wider buffer)"""
    a = Arena(shape, ld, dtype, guard_rows, device, col0)
    if fill is not None:
        a.view.copy_(fill.to(device=device, dtype=dtype))
    return a


def stray_count(a):
    """number of elements outside the view whose bits are no longer the NaN payload"""
    changed = a.raw != a.bits
    changed.view(a.rows + 2 * a.guard, a.ld)[a.guard:a.guard + a.rows, a.col0:a.col0 + a.cols] = False
    return int(changed.sum())


def assert_untouched(a, what="arena"):
    n = stray_count(a)
    assert n == 0, f"{what}: {n} elements outside the view changed"


def mismatches(got, ref):
    """number of elements of `got` that differ from `ref` by value (NaN differs from everything), and the first few (row, col) of them"""
    bad = got != ref.to(device=got.device, dtype=got.dtype)
    n = int(bad.sum())
    where = bad.nonzero()[:6].tolist() if n else []
    return n, where


# ------------------------------------------------------------------------------------------------ the shapes of tests/test_gpu_gemm_exact.py
NT_SMALL = [(8, 384, 32), (200, 136, 72), (136, 1001, 256), (40, 64, 2056), (129, 129, 8)]
NT_STAGGER = [(333, 260, 128), (700, 1001, 192)]
NT_PERSIST = [(4352, 4096, 128), (4352, 4096, 192)]
NT_PERSIST_320 = (5440, 4096, 128)
NT_QUAD = [(M, N, K) for M in (192, 256, 320) for N in (256, 512) for K in (128, 192, 448)]
NT_QUAD_ASM = [(M, N, 256) for M in (256, 320) for N in (256, 512)]    # 4 K tiles: the smallest count the generated asm K loop takes (fm = 4, 5)
NT_QUAD_RAGGED = (5000, 2048, 128)
NT_QUAD_RAGGED_320 = (8200, 2048, 128)                                # (the tile chooser picks 320-row tiles for this one)
NN = [(192, 256, 128), (320, 256, 256), (768, 256, 1024), (5000, 2048, 128)]
TN = [(128, 64, 200), (640, 1001, 328), (4096, 256, 256)]            # (Kc, M, N)
TN_QUAD = [(128, 192, 256), (192, 256, 512)]                          # fm = 3, fm = 4 (the K-major form has no 320-row tile)
TN_SPLITK = [(2048, 512, 768), (6464, 520, 264)]
TN_PAIR = (768, 256, 512, 1024)                                       # (M0, M1, N, Kc)
TN_MULTI = ([(512, 256), (256, 768)], 2048)
NT_SPLITK = [(704, 512, 8192), (100, 300, 640)]
NT_SPLITK_SLICE = (640, 256, 4096, 264)                               # (M, N, K, first column of `out` in a wider buffer)
SKINNY_M = (1, 2, 8)
SKINNY_NK = [(65, 64), (192, 64), (2304, 768), (768, 3072)]
SMALL_BATCH = [(5, 100, 32), (8, 12288, 128)]                         # (B, out, in)


def all_mnk():
    """every (M, N, K) product the GPU suite draws"""
    s = list(NT_SMALL) + list(NT_STAGGER) + list(NT_PERSIST) + [NT_PERSIST_320] + list(NT_QUAD) + list(NT_QUAD_ASM) + [NT_QUAD_RAGGED, NT_QUAD_RAGGED_320] + list(NN)
    s += [(M, N, Kc) for Kc, M, N in TN + TN_QUAD + TN_SPLITK]
    s += [(TN_PAIR[0], TN_PAIR[2], TN_PAIR[3]), (TN_PAIR[1], TN_PAIR[2], TN_PAIR[3])] + [(M, N, TN_MULTI[1]) for M, N in TN_MULTI[0]]
    s += list(NT_SPLITK) + [NT_SPLITK_SLICE[:3]] + [(M, N, K) for M in SKINNY_M for N, K in SKINNY_NK]
    s += [(o, i, B) for B, o, i in SMALL_BATCH] + [(B, i, o) for B, o, i in SMALL_BATCH]       # dW = dY^T X over B, dX = dY W over out
    return sorted(set(s))
