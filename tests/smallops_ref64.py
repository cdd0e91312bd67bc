"""fp64 / IEEE statements of the small kernels around the DiT blocks - token embedding forward and backward (csrc/rowops.hip), udm_rowgroup_sum_f32
(csrc/tokens.hip), the timestep embedding, SiLU forward and backward, the two casts of the gradient wire (csrc/rowops.hip), the bf16 transpose with its column
sums and the fp32 -> bf16 cast-transpose, single and multi (csrc/gemm.hip) - with their input families, bounds and mutants (CPU only).

The reference of tests/test_gpu_smallops_exact.py (GPU) and the subject of tests/test_smallops_ref64.py (CPU); the split follows rowops_ref64.py / gemm_ref64.py,
whose arenas, `rne_bf16` and `is_bf16_tie` are reused.

Exact kernels (both casts, both transposes, the embedding forward): the statement is IEEE arithmetic and the output equals it element for element, by value
(`mismatches`: a NaN must meet a NaN, +0 equals -0).
    cast_f32_bf16       rne_bf16(x);  with a scale  rne_bf16(fp32(rne_bf16(x)) * fp32(scale))   (the reference's compress hook: cast first, divide in bf16)
    cast_bf16_f32       fp32(x) * fp32(scale), one fp32 rounding
    embedding_fwd       E[clamp(id, 0, V - 1)] + Em[modality != 0], one fp32 addition
Family `edges` (fp32): bf16 rounding ties (5 of every 16 elements, both parities of the kept mantissa), one fp32 ulp either side of a tie, +-0, fp32 subnormals,
ties inside the bf16 subnormals, the largest finite bf16, fp32 values that round up to inf, +-inf, NaN, random values, and the bf16 values whose product with the
scale is a tie.  `scaled_tie_values` searches every finite bf16: a product with 1/3 is never a tie (the nearest mantissas are taken), with 1/6 and 1/8 the ties
lie where the subnormals drop bits.  `subnormal_mask` marks the elements that touch a subnormal anywhere in the statement: the GPU test asserts them under a name of their own.

Summing kernels (embedding_bwd dE / dEm, rowgroup_sum, colsum).  Family `ints`: integers in [-8, 8] times a power of two per column (gemm_ref64's
construction), the prefilled outputs too; every partial sum of a column is an integer below 2^24 in the column's unit (`partial_sums_exact`), so any order,
any atomics give the fp64 result exactly.  Family `gauss`: |got - ref| <= gamma_n sum|terms|, gamma_n = n u / (1 - n u), u = 2^-24, n the number of terms of
the element with the prefilled value counted - the bound of any summation order.

Bounded bf16 outputs (timestep embedding, SiLU forward and backward): rne_bf16(ref - E) <= got <= rne_bf16(ref + E) with
    timestep   E = FACTOR W 2^-24 (|ref| + 10 |arg| |d ref / d arg|)            (10: the frequency's exponent argument reaches ln 10^4)
    silu_fwd   E = FACTOR W 2^-24 |ref| (1 + |x| (1 - s)),  s = sigmoid(x)
    silu_bwd   E = FACTOR W 2^-24 |dy| (s + |x| s (1 - s)) (1 + |x| (1 - s)) + 2^-100     (fp32 exp(-x) overflows below -88: the kernel returns 0 for ~1e-39)
FACTOR = 4 as in rowops_ref64.  W is the worst ratio an fp32 restatement of the kernel's own formula (torch fp32 ops in the kernel's order, unrounded) reaches
against fp64 at FACTOR W = 1, rounded up to an integer; tests/test_smallops_ref64.py measures it again and asserts the constants below:
    W_TIMESTEP = 1 (measured 0.972 on sigma in [0, 7])   W_TIMESTEP_FAR = 2 (1.006 on sigma up to 1000)   W_SILU_FWD = 3 (2.257)   W_SILU_BWD = 3 (2.965)
The measurement runs over the elements whose reference is a normal number; the kernels' formulas are the ones in csrc/rowops.hip today: SiLU forward evaluates
x e^x as (x e^(x/2)) e^(x/2) below -80, where exp(-x) leaves the fp32 range while the result is still a normal bf16, and SiLU backward forms 1 - s as e s above 0
(with `1 - s` itself the restatement reaches 16.2: at x = 16.6, 1 + e^-x rounds to 1 and the whole x s (1 - s) term is lost).
`achieved(got, ref)` is the smallest e for which got lies in [rne_bf16(ref - e), rne_bf16(ref + e)]: the distance from ref to the rounding cell of got; the GPU
test records achieved / E.  Elements with more than one allowed value (`ambiguous`) are at most 2 % of a capped case, so the interval is no tolerance in disguise.
"""
import math

import torch

import gemm_ref64 as G

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
FACTOR = 4
W_TIMESTEP, W_TIMESTEP_FAR, W_SILU_FWD, W_SILU_BWD = 1, 2, 3, 3
W_MEASURED = dict(timestep=0.972, timestep_far=1.006, silu_fwd=2.257, silu_bwd=2.965)
SILU_DY = (1.0, 0.7421875, -3.0)
SILU_BWD_FLOOR = 2.0 ** -100
AMBIGUOUS_CAP = 0.02
SCALES = (1.0 / 3.0, 1.0 / 6.0, 1.0 / 8.0, 1.0)
CAST_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4099)
MIN_NORMAL = 2.0 ** -126
BLOCK_ROWS_EMB, BLOCK_ROWS_GROUP = 128, 512      # rows per block of embedding_bwd_kernel / rowgroup_sum_kernel

EMB_FWD_D, EMB_BWD_D, EMB_BWD_M = (4, 192, 260, 1024, 2048), (4, 192, 1024, 1028, 2048, 4096), (1, 7, 128, 129, 1000)
ROWGROUP = ((1, 4, 1), (513, 72, 3), (1100, 64, 32), (777, 768, 16))
TIMESTEP_DIMS, TIMESTEP_B = (2, 6, 7, 256), (1, 5, 64)
SIGMA_EDGE = (0.0, 1e-8, 1e-3, 6.9077)
TRANSPOSE = ((8, 8), (72, 136), (200, 72), (64, 64))
CAST_TRANSPOSE = ((65, 64), (67, 67), (130, 520), (8, 192))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def f32(v):
    """the python float that holds fp32(v)"""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------ rounding and comparison
def rne(x):
    """fp32 (or fp32-representable fp64) -> bf16, round to nearest even on the bits (gemm_ref64.rne_bf16), NaN to NaN"""
    x64 = x.to(F64)
    nan = torch.isnan(x64)
    y = G.rne_bf16(torch.where(nan, torch.zeros_like(x64), x64))
    return torch.where(nan, torch.full_like(y, float("nan")), y)


def round_bf16_64(x64):
    """ANY fp64 -> the nearest bf16 value (ties to even, subnormals kept, overflow to inf), as fp64: the ends of the intervals"""
    a = x64.abs()
    _, e = torch.frexp(a)
    q = torch.ldexp(torch.ones_like(a), torch.clamp(e - 8, min=-133))
    r = torch.round(a / q) * q
    r = torch.where(r >= 2.0 ** 128, torch.full_like(r, float("inf")), r)
    r = torch.where(torch.isfinite(a) & (a != 0), r, a)
    return torch.copysign(r, x64)


def mismatches(got, ref):
    """number of elements that differ by value - NaN equals NaN here, +0 equals -0 - and the first few indices.  (gemm_ref64.mismatches counts a NaN as different
    from everything, which is right for GEMM outputs that must never be NaN; the casts and the transposes must carry a NaN through, so they compare with this one.)"""
    g, r = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    bad = (g != r) & ~(torch.isnan(g) & torch.isnan(r))
    n = int(bad.sum())
    return n, (bad.nonzero()[:6].tolist() if n else [])


def subnormal_mask(*ts):
    """elements at which any of the tensors holds a non-zero magnitude below 2^-126"""
    m = None
    for t in ts:
        a = t.detach().cpu().to(F64).abs()
        k = (a > 0) & (a < MIN_NORMAL)
        m = k if m is None else m | k
    return m


def gamma(n):
    """n u / (1 - n u) (n a number or a tensor)"""
    nu = torch.as_tensor(n, dtype=F64) * U
    return nu / (1 - nu)


def sum_ratio(got, ref, A, n):
    """largest |got - ref| / (gamma_n A) over the elements (0 where got == ref; inf where got is not finite or a zero bound is missed)"""
    g, r = got.detach().cpu().to(F64), ref.to(F64)
    err = (g - r).abs()
    bound = gamma(n) * A
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf")))
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


# ------------------------------------------------------------------------------------------------ casts
def cast_f32_bf16_ref(x, scale=1.0, mutant=None):
    """bf16 statement of udm_cast_f32_bf16.  mutants: half_away, truncate (the rounding of the cast), scale_first (scale applied before the cast)"""
    s = f32(scale)

    def rnd(t32):
        if mutant in ("half_away", "truncate"):
            u = t32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            u = ((u + 0x8000) if mutant == "half_away" else u) >> 16
            y = torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(BF16)
            return torch.where(torch.isnan(t32), torch.full_like(y, float("nan")), y)
        return rne(t32)

    x = x.to(F32)
    if s == 1.0:
        return rnd(x)
    if mutant == "scale_first":
        return rnd((x.to(F64) * s).to(F32))            # 24 x 24 bits: exact in fp64, one rounding to fp32
    return rnd((rnd(x).to(F64) * s).to(F32))            # 8 x 24 bits: exact in fp64, one rounding to fp32 (subnormals kept)


def cast_bf16_f32_ref(x, scale=1.0):
    return (x.to(F64) * f32(scale)).to(F32)


def cast_subnormals(x, scale):
    """the elements of a cast_f32_bf16 case that meet a subnormal in the statement: the input, the cast value, the fp32 product or the result"""
    c = rne(x)
    p = (c.to(F64) * f32(scale)).to(F32)
    return subnormal_mask(x, c, p, rne(p))


def scaled_tie_values(scale):
    """(bf16-representable fp64 values v > 0 whose product fp32(v fp32(scale)) is a bf16 rounding tie, whether such values exist), by a search over every finite
    bf16.  The product of an 8-bit and a 24-bit mantissa is rarely one: among the normal products of 1/3 and 1/6 there is none, and what the search finds lies
    where the fp32 or bf16 subnormals drop bits (1/6, 1/8).  Without any (1/3) the four mantissas whose product comes nearest to a tie are returned."""
    s = f32(scale)
    if s == 1.0:
        return torch.zeros(0, dtype=F64), False
    v = all_finite_bf16().to(F64)
    v = v[v > 0]
    p = (v * s).to(F32)
    low = p.view(torch.int32).to(torch.int64) & 0xFFFF
    tie = (low == 0x8000) & (p != 0)
    if bool(tie.any()):
        return v[tie], True
    v = torch.arange(128, 256, dtype=F64)
    low = (v * s).to(F32).view(torch.int32).to(torch.int64) & 0xFFFF
    return v[torch.argsort((low - 0x8000).abs())[:4]], False


def _bits_f32(u):
    u = u & 0xFFFFFFFF
    return torch.where(u >= 0x80000000, u - 0x100000000, u).to(torch.int32).view(F32)


def edges(n, seed, scale=1.0):
    """fp32 [n]: the family of the module docstring; element i is of class (i + i // 16) % 16, so every alignment of a 4-element group meets every class"""
    g = _gen(seed * 1009 + n)
    i = torch.arange(n)
    cls = (i + i // 16) % 16
    sign = torch.randint(0, 2, (n,), generator=g) << 31
    hi = torch.randint(0x0080, 0x7F7F, (n,), generator=g) << 16           # a normal finite bf16 magnitude
    low = torch.randint(0, 0x10000, (n,), generator=g)
    u = hi | low                                                           # classes 14: any normal fp32
    tie = (cls % 4 == 0) | (cls == 13)
    u = torch.where(tie, hi | 0x8000, u)
    u = torch.where(cls == 1, hi | 0x8001, u)
    u = torch.where(cls == 2, hi | 0x7FFF, u)
    u = torch.where(cls == 3, torch.zeros_like(u), u)
    u = torch.where(cls == 5, torch.randint(1, 0x800000, (n,), generator=g), u)                       # fp32 subnormals
    u = torch.where(cls == 6, torch.full_like(u, 0x7F7F0000), u)
    u = torch.where(cls == 7, 0x7F7F8000 + torch.randint(0, 0x8000, (n,), generator=g), u)          # rounds up to inf
    u = torch.where(cls == 9, torch.full_like(u, 0x7F800000), u)
    u = torch.where(cls == 10, torch.full_like(u, 0x7FC00001), u)
    u = torch.where(cls == 15, (torch.randint(0, 0x80, (n,), generator=g) << 16) | 0x8000, u)         # ties inside the bf16 subnormals
    x = _bits_f32(u | sign)
    st, _ = scaled_tie_values(scale)
    if st.numel():
        pick = st[torch.randint(0, st.numel(), (n,), generator=g)]
        pick = torch.where(sign != 0, -pick, pick).to(F32)
        x = torch.where(cls == 11, pick, x)
    return x


def edges_bf16(n, seed):
    """bf16 [n] for pure data movement: every kind of bit pattern - NaN, inf, subnormals, both zeros"""
    g = _gen(seed * 31 + n)
    u = torch.randint(0, 0x10000, (n,), generator=g)
    special = torch.tensor([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0x0001, 0x807F, 0x7F7F])
    u = torch.where(torch.arange(n) % 5 == 0, special[torch.randint(0, 8, (n,), generator=g)], u)
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(BF16)


def tie_share(x):
    """share of exact bf16 rounding ties (gemm_ref64.is_bf16_tie, on the finite elements) among the elements, and whether both parities of the kept mantissa occur"""
    fin = torch.isfinite(x)
    t = fin & G.is_bf16_tie(torch.where(fin, x, torch.zeros_like(x)).to(F64))
    odd = (x.contiguous().view(torch.int32).to(torch.int64) >> 16) & 1
    return float(t.double().mean()), bool((t & (odd == 0)).any() and (t & (odd == 1)).any())


# ------------------------------------------------------------------------------------------------ summing families
def ints(M, d, seed, r=6):
    """(values fp64 [M, d], column exponents int64 [d]): integers in [-8, 8] times 2^(f_c); exact in bf16 and in fp32"""
    g = _gen(seed * 7919 + 13 * M + d)
    i = torch.randint(-8, 9, (M, d), generator=g)
    f = torch.randint(-r, r + 1, (d,), generator=g)
    return torch.ldexp(i.to(F64), f[None, :].expand(M, d)), f


def ints_like(shape, f, seed):
    """a prefilled output of the `ints` family: the same unit per column"""
    i = torch.randint(-8, 9, tuple(shape), generator=_gen(seed * 104729 + 7))
    return torch.ldexp(i.to(F64), f.expand(tuple(shape)))


def gauss(shape, seed, scale=1.0):
    return (torch.randn(tuple(shape), generator=_gen(seed * 15485863 + 1)) * scale).to(F32)


def partial_sums_exact(A, f):
    """A [.., d]: the sum of the magnitudes of every term of an element (prefilled value included), f the column exponents: every partial sum of every order is
    an integer of the column's unit below 2^24"""
    k = torch.ldexp(A, -f.expand(A.shape))
    return bool((k == k.round()).all()) and float(k.max()) < G.LIMIT


# ------------------------------------------------------------------------------------------------ embedding
def make_ids(M, V, seed, hot_id=None, hot_share=0.0, out_of_range=True):
    """int64 [M]: random rows of the table, a share of them `hot_id`, and - from M = 7 on - the ids -1, -100, V and V + 7 at rows 1, 3, M - 2 and M - 1"""
    g = _gen(seed * 613 + M + 3 * V)
    ids = torch.randint(0, V, (M,), generator=g)
    if hot_id is not None:
        if hot_share >= 1.0:
            ids[:] = hot_id
        elif hot_share > 0:
            ids[torch.rand(M, generator=g) < hot_share] = hot_id
        else:
            ids[ids == hot_id] = (hot_id + 1) % V if V > 1 else hot_id
    if out_of_range and M >= 7:
        ids[1], ids[3], ids[M - 2], ids[M - 1] = -1, -100, V, V + 7
    return ids


def make_modality(M, seed):
    """int64 [M] with values 0, 1 and 2 (2 counts as image, like every non-zero value)"""
    return torch.randint(0, 3, (M,), generator=_gen(seed * 389 + M))


EMB_V, EMB_HOT = 13, 5


def emb_case(family, d, M, share, seed=0, V=EMB_V, hot_id=EMB_HOT):
    """one embedding_bwd case: (ids, modality, dx, dE0, dEm0 - fp32 - and the column exponents of the `ints` family or None)"""
    ids = make_ids(M, V, seed + d, hot_id=hot_id, hot_share=share)
    mod = make_modality(M, seed + d)
    if family == "ints":
        dx, f = ints(M, d, seed + 1)
        dE0, dEm0 = ints_like((V, d), f, seed + 2), ints_like((2, d), f, seed + 3)
    else:
        dx, f = gauss((M, d), seed + 1), None
        dE0, dEm0 = gauss((V, d), seed + 2), gauss((2, d), seed + 3)
    return ids, mod, dx.to(F32), dE0.to(F32), dEm0.to(F32), f


def embedding_fwd_ref(ids, E, modality=None, Em=None):
    """fp32 [M, d]: E[clamp(id)] (+ Em[modality != 0]): a copy, or one IEEE fp32 addition"""
    x = E.to(F32)[ids.clamp(0, E.shape[0] - 1)]
    if Em is not None:
        x = x + Em.to(F32)[(modality != 0).long()]
    return x


def embedding_bwd_ref(ids, dx, dE0, modality=None, dEm0=None, mutant=None, hot_id=None):
    """dE = dE0 + scatter of the rows of dx with an id in [0, V) (others are dropped), dEm = dEm0 + the rows of dx by modality != 0 (every row): fp64, with the
    sums of the magnitudes A_* and the numbers of terms n_* (prefilled value included) for the `gauss` bound.  `hot_id` enters the mutants only."""
    M, d = dx.shape
    V = dE0.shape[0]
    t = dx.to(F64).clone()
    rows = torch.arange(M)
    ok = (ids >= 0) & (ids < V)
    idx = ids
    if mutant == "drop_block_last_row":
        ok = ok & (rows % BLOCK_ROWS_EMB != BLOCK_ROWS_EMB - 1)
    if mutant == "hot_twice":
        t = torch.where((ids == hot_id)[:, None], 2 * t, t)
    if mutant == "clamp_out_of_range":
        idx, ok = ids.clamp(0, V - 1), torch.ones(M, dtype=torch.bool)
    dE = dE0.to(F64).clone().index_add_(0, idx[ok], t[ok])
    if mutant == "cancelled_hot_garbage":               # a block whose hot rows sum to 0 stores something all the same
        for r0 in range(0, M, BLOCK_ROWS_EMB):
            h = (ids[r0:r0 + BLOCK_ROWS_EMB] == hot_id)
            if bool(h.any()):
                s = t[r0:r0 + BLOCK_ROWS_EMB][h].sum(0)
                dE[hot_id] += torch.where(s == 0, torch.ones_like(s), torch.zeros_like(s))
    out = dict(dE=dE, A_dE=dE0.to(F64).abs().index_add_(0, ids[ok & (ids >= 0) & (ids < V)], t[ok & (ids >= 0) & (ids < V)].abs()),
               n_dE=(1 + torch.bincount(ids[(ids >= 0) & (ids < V)], minlength=V)).to(F64)[:, None].expand(V, d))
    if dEm0 is not None:
        m = (modality != 0).long()
        if mutant == "modality_swapped":
            m = 1 - m
        out.update(dEm=dEm0.to(F64).clone().index_add_(0, m, dx.to(F64)), A_dEm=dEm0.to(F64).abs().index_add_(0, m, dx.to(F64).abs()),
                   n_dEm=(1 + torch.bincount(m, minlength=2)).to(F64)[:, None].expand(2, d))
    return out


def cancelling_hot_block(ids, dx, hot_id, V):
    """make the hot rows of the first 128-row block cancel exactly, in the kernel's own order: the block's rows become adjacent pairs (hot, hot) with dx and -dx;
    an odd row out gets another id.  Returns (ids, dx)."""
    ids, dx = ids.clone(), dx.clone()
    n = min(BLOCK_ROWS_EMB, ids.numel())
    other = (hot_id + 1) % V
    for r in range(0, n - 1, 2):
        ids[r], ids[r + 1] = hot_id, hot_id
        dx[r + 1] = -dx[r]
    if n % 2:
        ids[n - 1] = other
    ids[n:][ids[n:] == hot_id] = other
    return ids, dx


# ------------------------------------------------------------------------------------------------ rowgroup_sum
def make_groups(M, G_, run=37):
    """int64 [M]: runs of `run` rows whose indices walk through 0, -1, G (both outside [0, G)), 1, 2, .. G - 1 and round again, so that the first run - the only
    one of M = 1 - is summed into group 0; the run that covers row 511 also covers row 512 and has the index G - 1.  Every case hits groups 0 and G - 1."""
    k = torch.arange(M) // run
    g = torch.tensor([0, -1, G_] + list(range(1, G_)))[k % (G_ + 2)]
    if M > BLOCK_ROWS_GROUP:
        seam = k == (BLOCK_ROWS_GROUP - 1) // run
        g = torch.where(seam, torch.full_like(g, G_ - 1), g)
    return g


def rowgroup_ref(x, group, out0, mutant=None):
    """out0 + the sums of the rows of x by group, rows with an index outside [0, G) skipped: (ref, A, n) in fp64"""
    G_, d = out0.shape
    ok = (group >= 0) & (group < G_)
    keep = ok
    if mutant == "lose_seam_run" and x.shape[0] > BLOCK_ROWS_GROUP:
        s = BLOCK_ROWS_GROUP - 1
        lo, hi = s, s + 1
        while lo > 0 and group[lo - 1] == group[s]:
            lo -= 1
        while hi < x.shape[0] and group[hi] == group[s]:
            hi += 1
        keep = ok.clone()
        if hi > s + 1:
            keep[lo:hi] = False
    t = x.to(F64)
    ref = out0.to(F64).clone().index_add_(0, group[keep], t[keep])
    A = out0.to(F64).abs().index_add_(0, group[ok], t[ok].abs())
    n = (1 + torch.bincount(group[ok], minlength=G_)).to(F64)[:, None].expand(G_, d)
    return ref, A, n


# ------------------------------------------------------------------------------------------------ transposes
def colsum_ref(x, c0, mutant=None):
    """c0 + the column sums of x [R, C]: (ref, A, n) in fp64"""
    t = x.to(F64)
    if mutant == "skip_last8":
        t = t[:-8]
    return c0.to(F64) + t.sum(0), c0.to(F64).abs() + x.to(F64).abs().sum(0), float(x.shape[0] + 1)


def transpose_ref(x, mutant=None):
    y = x.t().clone()
    if mutant == "tile_rows_swapped":
        y[[0, 1]] = y[[1, 0]]
    return y


def cast_transpose_ref(w):
    """(out bf16 [R, C], out_t bf16 [C, R])"""
    o = rne(w)
    return o, o.t().clone()


# ------------------------------------------------------------------------------------------------ bounded bf16 outputs
def interval(ref, E):
    return round_bf16_64(ref - E), round_bf16_64(ref + E)


def outside(got, ref, E):
    """bool: the elements of the bf16 tensor `got` outside [rne_bf16(ref - E), rne_bf16(ref + E)] (a NaN is outside)"""
    g = got.detach().cpu().to(F64)
    lo, hi = interval(ref, E)
    return ~((g >= lo) & (g <= hi))


def ambiguous(ref, E):
    """share of the elements with more than one allowed value"""
    lo, hi = interval(ref, E)
    return float((lo != hi).double().mean())


def achieved(got, ref):
    """per element, the distance from ref to the rounding cell of the bf16 value got (0 inside it): the least E that admits got.  inf for a NaN or a wrong inf."""
    gb = got.detach().cpu().contiguous()
    g = gb.to(F64)
    b = gb.view(torch.int16).to(torch.int64) & 0xFFFF
    mag, neg = b & 0x7FFF, (b >> 15) == 1

    def val(m):
        return (m.clamp(0, 0x7F80) << 16).to(torch.int32).view(F32).to(F64)

    v = val(mag)
    hi = torch.where(mag + 1 >= 0x7F80, v + (v - val(mag - 1)) / 2, (v + val(mag + 1)) / 2)      # past the largest finite: the overflow threshold
    lo = torch.where(mag == 0, -val(torch.ones_like(mag)) / 2, (v + val(mag - 1)) / 2)
    r = torch.where(neg, -ref, ref)
    need = torch.clamp(torch.maximum(lo - r, r - hi), min=0.0)
    same = g == round_bf16_64(ref)
    need = torch.where(same, torch.zeros_like(need), need)
    return torch.where(torch.isfinite(g) | same, need, torch.full_like(need, float("inf")))


def worst_ratio(got, ref, E):
    """largest achieved / E (0 where nothing is needed, inf where a zero E is missed)"""
    a = achieved(got, ref)
    q = torch.where(a == 0, torch.zeros_like(a), a / E)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


def sigmas(B, family, seed):
    """fp32 [B]: `schedule` - 0, 1e-8, 1e-3 and the schedule's end 6.9077 in front of uniform draws on [0, 7]; `far` - 1000 (and uniform draws up to it)"""
    u = torch.rand(B, generator=_gen(seed * 211 + B))
    if family == "far":
        s = u * 1000.0
        s[0] = 1000.0
        return s.to(F32)
    s = u * 7.0
    k = min(B, len(SIGMA_EDGE))
    s[:k] = torch.tensor(SIGMA_EDGE[(4 - k) % 4:][:k] if B < 4 else SIGMA_EDGE)
    return s.to(F32)


def timestep_ref(sigma, dim, mutant=None):
    """(ref fp64 [B, dim], S = |ref| + 10 |arg| |d ref / d arg|): cos(sigma f_j) | sin(sigma f_j) | 0 for an odd dim, f_j = exp(-ln(10^4) j / half)"""
    half = dim // 2
    B = sigma.numel()
    jj = torch.arange(half, dtype=F64)
    den = half - 1 if mutant == "half_minus_1" else half
    arg = sigma.to(F64)[:, None] * torch.exp(-math.log(10000.0) * jj / den)[None]
    c, s = torch.cos(arg), torch.sin(arg)
    if mutant == "cos_sin_swapped":
        c, s = s, c
    tail = torch.zeros(B, dim - 2 * half, dtype=F64)
    ref = torch.cat([c, s, tail + (1.0 if mutant == "odd_tail_nonzero" else 0.0)], -1)
    S = torch.cat([c.abs() + 10 * arg.abs() * s.abs(), s.abs() + 10 * arg.abs() * c.abs(), tail], -1)
    return ref, S


def timestep_f32(sigma, dim):
    """the kernel's formula in torch fp32 ops, unrounded (tests/fake_kernels.py::timestep_embedding)"""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=F32) / half)
    args = sigma[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args), torch.zeros(sigma.numel(), dim - 2 * half)], -1)


def timestep_E(S, W=W_TIMESTEP):
    return FACTOR * W * U * S


def _sig(x64):
    """(sigmoid(x), 1 - sigmoid(x)) without cancellation"""
    e = torch.exp(-x64.abs())
    a, b = 1 / (1 + e), e / (1 + e)
    pos = x64 >= 0
    return torch.where(pos, a, b), torch.where(pos, b, a)


def silu_ref(x):
    """(ref, S = |ref| (1 + |x| (1 - s))) of x sigmoid(x), fp64"""
    x = x.to(F64)
    s, c = _sig(x)
    ref = x * s
    return ref, ref.abs() * (1 + x.abs() * c)


def silu_f32(x):
    """the kernel's formula in torch fp32 ops, unrounded: v / (1 + exp(-v)); below -80 (v e^(v / 2)) e^(v / 2)"""
    v = x.to(F32)
    h = torch.exp(0.5 * v)
    return torch.where(v < -80.0, (v * h) * h, v / (1 + torch.exp(-v)))


def silu_E(S, W=W_SILU_FWD):
    return FACTOR * W * U * S


def silu_bwd_ref(x, dy, mutant=None):
    """(ref, S) of dy (s + x s (1 - s)); S = |dy| (s + |x| s (1 - s)) (1 + |x| (1 - s))"""
    x, dy = x.to(F64), dy.to(F64)
    s, c = _sig(x)
    g = s if mutant == "no_x_term" else s + x * s * c
    return dy * g, dy.abs() * (s + x.abs() * s * c) * (1 + x.abs() * c)


def silu_bwd_f32(x, dy):
    """the kernel's formula in torch fp32 ops, unrounded: 1 - s is e s above 0"""
    v = x.to(F32)
    e = torch.exp(-v)
    s = 1 / (1 + e)
    return dy.to(F32) * (s + v * s * torch.where(v > 0, e * s, 1 - s))


def silu_bwd_E(S, W=W_SILU_BWD):
    return FACTOR * W * U * S + SILU_BWD_FLOOR


def silu_dys(n):
    """the output gradients of the SiLU backward sweep: three constants and one random bf16 tensor"""
    return [torch.full((n,), v, dtype=BF16) for v in SILU_DY] + [torch.randn(n, generator=_gen(4711)).to(BF16)]


def all_finite_bf16():
    """every finite bf16 bit pattern (both zeros, the subnormals), bf16 [65280]"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF16)


def measure_W(f32_value, ref, S, floor=0.0):
    """worst |fp32 restatement - ref| / (2^-24 S + floor) over the elements with |ref| >= 2^-126: the W of the module docstring before it is rounded up.
    (Below the normal range neither fp32 nor bf16 carries a relative error; there the interval is decided by the rounding to the subnormal grid.)"""
    err = (f32_value.to(F64) - ref).abs()
    q = torch.where((err == 0) | (ref.abs() < MIN_NORMAL), torch.zeros_like(err), err / (U * S + floor))
    return float(q.max())
