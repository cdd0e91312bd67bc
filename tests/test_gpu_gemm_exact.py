"""Every GEMM dispatch path against fp64, element for element, on operands whose product is exact - out of NaN arenas.

Operands (tests/gemm_ref64.py): A[i, k] = a_ik 2^(e_i), B[j, k] = b_jk 2^(f_j) with small integers a, b.  Every fp32 partial sum is then exact, in any order,
through any K split, workspace or atomic: an fp32 output must EQUAL the fp64 reference, a bf16 output its round-to-nearest-even rounding (8 % of the results
are exact ties: round-half-away fails).  The same holds through the bias add, beta = 1 and the GELU' product with its fused column sums (aux from
{0, +-0.5, +-1, +-2}); the GELU epilogue is held per element to |got - ref64| <= 2^-8 |ref64| + 2^-20.  tests/test_gemm_ref64.py shows on the CPU that the
reference alone meets these conditions and that the comparator rejects a dropped K element, round-half-away and a transposed fragment.

Buffers: A, B, C, aux, bias gradients live as strided views inside allocations filled with a NaN of known payload (384 guard rows before and after, NaN in the
pad columns [cols, ld)).  An operand read past K or past the last row puts a NaN into the result; beta = 0 reading C does too (C starts as NaN); a store
outside C changes known bits (`stray_count`).  The library's split-K scratch is filled with NaN before every call: a reduce pass over a slice nobody wrote
shows up as NaN.  Nothing here reads or writes outside an allocation.

Comparisons are by value: NaN differs from everything, +0 equals -0.  Every path records its count of mismatching elements (asserted 0), its stray-store
count and, for the GELU epilogues, the excess over the bound in the parity ledger (tests/ledger.py)."""
import functools

import pytest
import torch

import gemm_ref64 as R
import ledger

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
NAN = float("nan")
TEST = "gemm_exact"


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def up(n, m):
    return (n + m - 1) // m * m


@functools.lru_cache(maxsize=4)
def problem(M, N, Kd, family):
    """the drawn problem of a shape, shared by the tests that use it (never modified): family 'plain' | 'bias' | 'cols' (EPI_DGELU) | 'gelu'"""
    seed = M * 31 + N * 7 + Kd
    if family == "gelu":
        return R.exact_gelu_operands(M, N, Kd, seed=seed)
    if family == "cols":
        return R.exact_operands(M, N, Kd, seed=seed, row_scales="cols")
    if family == "plain":
        p = problem(M, N, Kd, "bias")
        return p if p.r == 6 else R.exact_operands(M, N, Kd, seed=seed)   # (where the bias family had to narrow its scales, the plain product keeps the full range)
    return R.exact_operands(M, N, Kd, seed=seed, bias=True)


def poison_scratch(K):
    """the library's split-K workspace, sized beyond every shape here by one request and filled with NaN"""
    ws = K._scratch(1 << 24, torch.empty(0, device=DEV).device)      # (the device as the wrappers see it on their operands: the scratch is kept per device)
    ws.fill_(NAN)
    return ws


def place(x, *, pad=8, mult=8, ld=None, dtype=None, col0=0, guard=R.GUARD_ROWS):
    """a CPU operand as a view in a NaN arena on the device: row stride = cols rounded up to `mult` plus `pad` NaN columns"""
    dtype = dtype or x.dtype
    rows, cols = x.shape
    ld = ld if ld is not None else up(col0 + cols, mult) + pad
    return R.arena((rows, cols), ld, dtype, guard_rows=guard, device=DEV, fill=x, col0=col0)


def blank(rows, cols, dtype, *, pad=None, mult=None, ld=None, col0=0):
    """an output arena: the view itself starts as NaN as well"""
    mult = mult or (8 if dtype == BF16 else 4)
    pad = mult if pad is None else pad
    ld = ld if ld is not None else up(col0 + cols, mult) + pad
    return R.arena((rows, cols), ld, dtype, device=DEV, col0=col0)


class Report:
    """collects what a case found; `done` asserts that nothing was found"""

    def __init__(self, path, shape):
        self.path, self.shape, self.faults = path, "x".join(str(s) for s in shape), []

    def equal(self, what, got, ref):
        n, where = R.mismatches(got, ref)
        ledger.record(TEST, f"{self.path} {self.shape} {what} mismatches", n, 0)
        if n:
            self.faults.append(f"{what}: {n} of {got.numel()} elements differ from the reference, first (row, col) {where}")

    def untouched(self, what, *arenas):
        torch.cuda.synchronize()
        n = sum(R.stray_count(a) for a in arenas)
        ledger.record(TEST, f"{self.path} {self.shape} {what} stray elements", n, 0)
        if n:
            self.faults.append(f"{what}: {n} arena elements outside the outputs changed")

    def gelu(self, what, got, ref64, allow):
        """per-element bound of the GELU epilogues; `allow` = twice the excess of torch's own fp32 evaluation over the same bound where that is positive"""
        ref64 = ref64.to(got.device).expand_as(got)
        finite = bool(torch.isfinite(got.float()).all())
        ex = R.gelu_excess(got, ref64) if finite else float("inf")
        ledger.record(TEST, f"{self.path} {self.shape} {what} excess over 2^-8 |ref| + 2^-20", ex, allow, note="negative: inside the bound")
        ledger.record(TEST, f"{self.path} {self.shape} {what} worst |got - ref| / (2^-8 |ref| + 2^-20)", R.gelu_ratio(got, ref64) if finite else float("inf"))
        if not finite or ex > allow:
            self.faults.append(f"{what}: excess {ex:.3e} over the bound (allowed {allow:.3e}), finite={finite}")

    def workspace(self, what, ws, n):
        """evidence of the path: a workspace entry point must have filled the first `n` elements of the (NaN-filled) scratch with partial sums; n = 0: a call
        that must not split (a fallback, or an entry point without a workspace) leaves every element NaN"""
        torch.cuda.synchronize()
        ok = bool(torch.isfinite(ws[:n]).all()) if n else not bool(torch.isfinite(ws).any())
        ledger.record(TEST, f"{self.path} {self.shape} {what} workspace use as planned", 0 if ok else 1, 0)
        if not ok:
            self.faults.append(f"{what}: " + (f"the first {n} workspace elements were not all written: the split-K path was not taken" if n else "the scratch was written by a call that must not split"))

    def done(self):
        assert not self.faults, f"{self.path} {self.shape}:\n  " + "\n  ".join(self.faults)


@functools.lru_cache(maxsize=1)
def gelu_allowance():
    """(for C, for aux): 0 where torch's fp32 gelu / gelu' rounded to bf16 stays inside the bound on the sweep, twice its worst excess where it does not"""
    ey, eg = R.torch_gelu_excess()
    ledger.record(TEST, "torch fp32 gelu(tanh) -> bf16: excess over the bound on every bf16 in [-100, 100]", ey)
    ledger.record(TEST, "torch fp32 gelu'(tanh) -> bf16: excess over the bound on every bf16 in [-100, 100]", eg)
    return max(0.0, 2 * ey), max(0.0, 2 * eg)


# ------------------------------------------------------------------------------------------------ NT
VARIANTS = ("none_bf16", "none_f32", "bias_bf16", "bias_f32", "gelu", "dgelu_bf16", "dgelu_f32", "beta1")


def nt_case(K, rep, M, N, Kd, variant, *, narrow=False):
    """one gemm_nt call on a drawn problem in arenas; `narrow`: leading dimensions of C / aux that only the element-wise epilogue accepts (not multiples of 4)"""
    call = K.gemm_nt
    out_f32 = variant.endswith("f32") or variant == "beta1"
    cd = F32 if out_f32 else BF16
    ldc = dict(ld=N + (3 if (N + 3) % 4 else 5)) if narrow else {}
    ws = poison_scratch(K)
    if variant == "gelu":
        p, u = problem(M, N, Kd, "gelu")
    else:
        p = problem(M, N, Kd, "cols" if variant.startswith("dgelu") else "plain" if variant.startswith("none") else "bias")
    a, b, c = place(p.A), place(p.B), blank(M, N, cd, **ldc)
    arenas = [a, b, c]
    if variant.startswith("none"):
        call(a.view, b.view, out=c.view)
        rep.equal(variant, c.view, p.ref if out_f32 else R.rne_bf16(p.ref))
    elif variant.startswith("bias"):
        bias = place(p.bias[None, :], mult=4, pad=4)
        arenas.append(bias)
        call(a.view, b.view, out=c.view, epilogue=K.EPI_BIAS, bias=bias.view[0])
        rep.equal(variant, c.view, p.ref_bias if out_f32 else R.rne_bf16(p.ref_bias))
    elif variant == "beta1":
        c0, ref = R.exact_c0(p, seed=M + N)
        c.view.copy_(c0)
        call(a.view, b.view, out=c.view, beta=1.0)
        rep.equal(variant, c.view, ref)
    elif variant == "gelu":
        bias, aux = place(p.bias[None, :], mult=4, pad=4), blank(M, N, BF16, **ldc)
        arenas += [bias, aux]
        call(a.view, b.view, out=c.view, epilogue=K.EPI_BIAS_GELU, bias=bias.view[0], aux=aux.view)
        ay, ag = gelu_allowance()
        rep.gelu("gelu C", c.view, R.gelu64(u), ay)
        rep.gelu("gelu aux", aux.view, R.dgelu64(u), ag)
    else:
        auxv, d0, cref, dbref = R.exact_dgelu(p, seed=M + N + 1, out_f32=out_f32)
        aux, db = place(auxv, **({"ld": ldc["ld"]} if narrow else {})), place(d0[None, :], mult=4, pad=4)
        arenas += [aux, db]
        call(a.view, b.view, out=c.view, epilogue=K.EPI_DGELU, aux=aux.view, bias=db.view[0])
        rep.equal(variant, c.view, cref)
        rep.equal(variant + " dbias", db.view[0], dbref)
    rep.untouched(variant, *arenas)
    rep.workspace(variant, ws, 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,N,Kd", R.NT_SMALL)
def test_nt_small_kernel(K, M, N, Kd, variant):
    """128 x 128 register-staged kernel: every shape here has M < 192, or N < 192, or K % 64 != 0, or K < 128 (gemm_choose_tile of csrc/gemm_plan.h returns 0).  K tails of 8
    (K = 72, 2056, 8: K % 64 == 8) with NaN right behind K; M, N ragged against the 128-wide tile ((129, 129): one row / column in the second tile)."""
    rep = Report("nt 128x128", (M, N, Kd))
    nt_case(K, rep, M, N, Kd, variant)
    rep.done()


@pytest.mark.parametrize("variant", ("none_bf16", "none_f32", "bias_bf16", "gelu", "dgelu_bf16", "dgelu_f32", "beta1"))
def test_nt_small_kernel_narrow_ldc(K, variant):
    """ldc (and ldaux) not a multiple of 4: only the element-by-element stores of the 128 x 128 kernel's epilogue accept it (n_vec_ok false)"""
    rep = Report("nt 128x128 narrow ldc", (200, 136, 72))
    nt_case(K, rep, 200, 136, 72, variant, narrow=True)
    rep.done()


@pytest.mark.parametrize("tile", [192, 256, 320, 0])
@pytest.mark.parametrize("M,N,Kd", R.NT_STAGGER)
def test_nt_stagger_kernels(K, tile, M, N, Kd):
    """LDS-DMA stagger kernels forced per tile family (gemm_set_tile; 0 = the 128 x 128 kernel on a shape it would not get by itself): K % 64 == 0 and
    K >= 128, so gemm_choose_tile obeys the forced tile; ragged M and N in the last tile row / column; two and three K tiles; fewer than 256 tiles: one block per tile."""
    rep = Report(f"nt stagger tile {tile}", (M, N, Kd))
    K.gemm_set_tile(tile)
    try:
        for variant in VARIANTS:
            nt_case(K, rep, M, N, Kd, variant)
    finally:
        K.gemm_set_tile(-1)
    rep.done()


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("tile,M,N,Kd", [(256,) + s for s in R.NT_PERSIST] + [(320,) + R.NT_PERSIST_320])
def test_nt_persistent_wide(K, tile, M, N, Kd, persist):
    """Persistent wide form: 17 x 16 = 272 whole tiles (> 256), M % tile == 0, N % 256 == 0, K / 64 >= 2, ldc % 8 == 0, ldaux % 8 == 0
    (gemm_persistent_wide_ok), even and odd K-tile counts.  The tile is forced: gemm_choose_tile by itself prefers one ragged round of 320-row tiles at M = 4352.
    persist = 0: the same shapes with one block per tile (gemm_set_persist)."""
    rep = Report(f"nt tile {tile} " + ("persistent" if persist else "one block per tile"), (M, N, Kd))
    K.gemm_set_tile(tile)
    K.gemm_set_persist(persist)
    try:
        for variant in ("none_bf16", "bias_f32", "gelu", "dgelu_bf16"):
            nt_case(K, rep, M, N, Kd, variant)
    finally:
        K.gemm_set_persist(1)
        K.gemm_set_tile(-1)
    rep.done()


@pytest.mark.parametrize("asm", [1, 0])
@pytest.mark.parametrize("M,N", [(M, N) for M in (192, 256, 320) for N in (256, 512)])
def test_nt_quad_one_wave_per_simd(K, M, N, asm):
    """One-wave-per-SIMD kernel under gemm_set_quad(2): M = 192 / 256 / 320 is exactly one tile row of fm = 3 / 4 / 5 (gemm_quad_whole_fm: N % 256 == 0,
    K % 64 == 0, K >= 128; 320 is no multiple of 192 or 256, 256 none of 192), K tiles 2 / 3 / 7 - which all run the C++ K loop whatever `asm` says: the
    generated asm loop is taken for at least 4 K tiles and an even count, on the 256- and 320-row tiles.  K = 256 (R.NT_QUAD_ASM: 4 K tiles, the smallest count
    it takes) is where asm = 1 and asm = 0 differ (tests/test_gemm_plan.py lists the plan of every case here)."""
    rep = Report(f"nt quad asm={asm}", (M, N))
    K.gemm_set_quad(2)
    K.debug_set("gemm_quad_asm", asm)
    try:
        for Kd in (128, 192, 448) + tuple(k for m, n, k in R.NT_QUAD_ASM if (m, n) == (M, N)):
            rep.shape = f"{M}x{N}x{Kd}"
            for variant in ("none_bf16", "bias_bf16", "none_f32"):
                nt_case(K, rep, M, N, Kd, variant)
    finally:
        K.debug_set("gemm_quad_asm", -1)
        K.gemm_set_quad(1)
    rep.done()


@pytest.mark.parametrize("M,N,Kd", [R.NT_QUAD_RAGGED, R.NT_QUAD_RAGGED_320])
def test_nt_quad_ragged_last_tile_row(K, M, N, Kd):
    """Ragged 320-row tiles (fm = -5): udm_gemm_nt_bf16 takes them when gemm_choose_tile picks 320 for one round of 128..256 tiles with M % 320 != 0.
    (8200, 2048, 128): 26 x 8 = 208 tiles in one round where 192- / 256-row tiles need two -> the ragged form; the rows behind M are guard rows.
    (5000, 2048, 128): gemm_choose_tile prefers one round of 192-row tiles (27 x 8 = 216), so NT runs the ragged 8-wave kernel there; gemm_nn (test_nn) is where
    this shape takes fm = -5."""
    rep = Report("nt ragged 320-row tiles", (M, N, Kd))
    K.gemm_set_quad(2)
    try:
        for variant in ("none_bf16", "bias_bf16"):
            nt_case(K, rep, M, N, Kd, variant)
    finally:
        K.gemm_set_quad(1)
    rep.done()


# ------------------------------------------------------------------------------------------------ NN
@pytest.mark.parametrize("M,N,Kd", R.NN)
def test_nn(K, M, N, Kd):
    """gemm_nn / gemm_nn_splitk: fm = 3 (192), fm = 5 (320), fm = 3 with 4 tiles over 16 K tiles (768 x 256 x 1024: gemm_nn_splitk cuts K 4 ways through the
    workspace), and 16 x 8 = 128 ragged 320-row tiles (5000 x 2048: fm = -5; the split form falls back to the plain one)."""
    assert K.gemm_nn_ok(M, N, Kd)
    rep = Report("nn", (M, N, Kd))
    p = problem(M, N, Kd, "plain")
    ref = R.rne_bf16(p.ref)
    for name, fn in (("gemm_nn", K.gemm_nn), ("gemm_nn_splitk", K.gemm_nn_splitk)):
        ws = poison_scratch(K)
        a, b, c = place(p.A), place(R.nn_layout(p.B), pad=16), blank(M, N, BF16)
        fn(a.view, b.view, c.view)
        rep.equal(name, c.view, ref)
        rep.untouched(name, a, b, c)
        rep.workspace(name, ws, 4 * M * N if name == "gemm_nn_splitk" and (M, N, Kd) == (768, 256, 1024) else 0)
    rep.done()


# ------------------------------------------------------------------------------------------------ TN
def tn_operands(p):
    return place(R.tn_layout(p.A)), place(R.tn_layout(p.B), pad=16)


def tn_check(K, rep, name, fn, p, beta, *, contiguous=False, slices=0):
    ws = poison_scratch(K)
    a, b = tn_operands(p)
    c = blank(p.M, p.N, F32, ld=p.N) if contiguous else blank(p.M, p.N, F32)
    ref = p.ref
    if beta:
        c0, ref = R.exact_c0(p, seed=p.M + p.N + 2)
        c.view.copy_(c0)
    fn(a.view, b.view, c.view, beta=float(beta))
    rep.equal(f"{name} beta={beta}", c.view, ref)
    rep.untouched(f"{name} beta={beta}", a, b, c)
    rep.workspace(f"{name} beta={beta}", ws, slices * p.M * p.N)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("Kc,M,N", R.TN)
def test_tn(K, Kc, M, N, beta):
    """gemm_tn on the 8-wave K-major kernels (N % 256 != 0, or too few tiles for the quad kernel in auto mode): a 192-row tile for M <= 192, ragged M and N,
    and (4096, 256, 256): one tile over 64 K tiles, which at beta = 1 is cut 4 ways with fp32 atomics into C (tiles * sk * 2 <= 32, >= 16 K tiles a slice)."""
    rep = Report("tn", (Kc, M, N))
    tn_check(K, rep, "gemm_tn", K.gemm_tn, problem(M, N, Kc, "plain"), beta)
    rep.done()


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("Kc,M,N", R.TN_QUAD)
def test_tn_quad(K, Kc, M, N, beta):
    """gemm_tn on the one-wave-per-SIMD K-major kernel under gemm_set_quad(2): M = 192 -> fm = 3, M = 256 -> fm = 4 (gemm_quad_whole_fm with fm_max = 4: the K-major form has no 320-row tile)"""
    rep = Report("tn quad", (Kc, M, N))
    K.gemm_set_quad(2)
    try:
        tn_check(K, rep, "gemm_tn", K.gemm_tn, problem(M, N, Kc, "plain"), beta)
    finally:
        K.gemm_set_quad(1)
    rep.done()


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("Kc,M,N", R.TN_SPLITK)
def test_tn_splitk_workspace(K, Kc, M, N, beta):
    """gemm_tn_splitk: (2048, 512, 768) = 6 quad tiles over 32 K tiles -> 4 slices; (6464, 520, 264) = 6 ragged 8-wave tiles over 101 K tiles -> 12 uneven
    slices.  The workspace holds NaN before the call."""
    rep = Report("tn splitk", (Kc, M, N))
    tn_check(K, rep, "gemm_tn_splitk", K.gemm_tn_splitk, problem(M, N, Kc, "plain"), beta, contiguous=True, slices=4 if Kc == 2048 else 12)
    rep.done()


@pytest.mark.parametrize("beta", [0, 1])
def test_tn_pair_workspace(K, beta):
    """gemm_tn_pair: (768 + 256) / 256 x 512 / 256 = 8 tiles over 16 K tiles -> 2 slices through the (NaN-filled) workspace, one reduce pass per output"""
    M0, M1, N, Kc = R.TN_PAIR
    assert K.gemm_tn_pair_ok(M0, M1, N, Kc)
    rep = Report("tn pair", R.TN_PAIR)
    ws = poison_scratch(K)
    ps = [problem(M0, N, Kc, "plain"), problem(M1, N, Kc, "plain")]
    ops, outs, refs = [], [], []
    for i, p in enumerate(ps):
        ops.append(tn_operands(p))
        c = blank(p.M, N, F32, ld=N)
        ref = p.ref
        if beta:
            c0, ref = R.exact_c0(p, seed=40 + i)
            c.view.copy_(c0)
        outs.append(c)
        refs.append(ref)
    K.gemm_tn_pair(ops[0][0].view, ops[0][1].view, outs[0].view, ops[1][0].view, ops[1][1].view, outs[1].view, beta=float(beta))
    for i in (0, 1):
        rep.equal(f"out{i} beta={beta}", outs[i].view, refs[i])
    rep.untouched(f"beta={beta}", *outs, *[x for o in ops for x in o])
    rep.workspace(f"beta={beta}", ws, 2 * (M0 + M1) * N)
    rep.done()


@pytest.mark.parametrize("beta", [0, 1])
def test_tn_multi_workspace(K, beta):
    """gemm_tn_multi: 2 + 3 = 5 tiles of two problems over K = 2048 (32 K tiles) -> 4 slices, one reduce pass over both outputs"""
    shapes, Kc = R.TN_MULTI
    rep = Report("tn multi", (Kc,) + tuple(x for s in shapes for x in s))
    ws = poison_scratch(K)
    probs, keep, refs = [], [], []
    for i, (M, N) in enumerate(shapes):
        p = problem(M, N, Kc, "plain")
        a, b = tn_operands(p)
        c = blank(M, N, F32, ld=N)
        ref = p.ref
        if beta:
            c0, ref = R.exact_c0(p, seed=50 + i)
            c.view.copy_(c0)
        probs.append((a.view, b.view, c.view))
        keep += [a, b, c]
        refs.append(ref)
    assert K.gemm_tn_multi(probs, beta=float(beta))
    for i, ref in enumerate(refs):
        rep.equal(f"out{i} beta={beta}", probs[i][2], ref)
    rep.untouched(f"beta={beta}", *keep)
    rep.workspace(f"beta={beta}", ws, 4 * sum(M * N for M, N in shapes))
    rep.done()


# ------------------------------------------------------------------------------------------------ NT split-K
@pytest.mark.parametrize("M,N,Kd,col0", [s + (0,) for s in R.NT_SPLITK] + [R.NT_SPLITK_SLICE])
def test_nt_splitk(K, M, N, Kd, col0):
    """gemm_nt_splitk: (704, 512, 8192) = 3 x 2 tiles of 320 x 256 over 128 K tiles -> 16 slices, ragged last tile row; (100, 300, 640): M < 320 falls back to
    gemm_nt; (640, 256, 4096) with `out` the columns [264, 520) of a wider buffer: 2 tiles over 64 K tiles -> 8 slices, the reduce pass honours ldc."""
    rep = Report("nt splitk", (M, N, Kd, col0))
    ws = poison_scratch(K)
    p = problem(M, N, Kd, "plain")
    a, b = place(p.A), place(p.B)
    c = blank(M, N, BF16, col0=col0, ld=up(col0 + N, 8) + 264 if col0 else None)
    K.gemm_nt_splitk(a.view, b.view, c.view)
    rep.equal("gemm_nt_splitk", c.view, R.rne_bf16(p.ref))
    rep.untouched("gemm_nt_splitk", a, b, c)
    rep.workspace("gemm_nt_splitk", ws, {8192: 16, 4096: 8, 640: 0}[Kd] * M * N)
    rep.done()


# ------------------------------------------------------------------------------------------------ skinny GEMM (decode.hip)
@pytest.mark.parametrize("N,Kd", R.SKINNY_NK)
@pytest.mark.parametrize("M", R.SKINNY_M)
def test_skinny(K, M, N, Kd):
    """gemm_skinny: N = 65 and 192 (not multiples of 128; 65 leaves one column in the third 32-column wave tile) against a weight shadow whose rows behind N
    are NaN, K = 64 (no split), 768 and 3072 (K split over workgroups through the NaN-filled workspace); every epilogue it accepts, both output types."""
    rep = Report("skinny", (M, N, Kd))
    ay, _ = gelu_allowance()
    for epi in ("none", "bias", "gelu"):
        for cd in (BF16, F32):
            what = f"{epi} {'f32' if cd == F32 else 'bf16'}"
            ws = poison_scratch(K)
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
            K.gemm_skinny(a.view, w.view, out=c.view, **kw)
            if epi == "gelu":
                rep.gelu(what, c.view, R.gelu64(u), ay)
            else:
                ref = p.ref if epi == "none" else p.ref_bias
                rep.equal(what, c.view, ref if cd == F32 else R.rne_bf16(ref))
            rep.untouched(what, *arenas)
            rep.workspace(what, ws, 2 * M * N if K.skinny_ws_elems(M, N, Kd) else 0)      # (K = 768, 3072: at least two slices; K = 64: no split)
    rep.done()


# ------------------------------------------------------------------------------------------------ small-batch Linear backward
@pytest.mark.parametrize("B,out,inp", R.SMALL_BATCH)
def test_small_batch_linear_bwd(K, B, out, inp):
    """udm_small_batch_linear_bwd on integer operands (|.| <= 8): dW = dY^T X (overwritten, at most 8 terms), db += colsum(dY), dX += dY W (at most 12288 terms of
    magnitude <= 64: below 2^24) are exact whatever the order of the atomics; db and dX start from integers."""
    rep = Report("small_batch_linear_bwd", (B, out, inp))
    g = torch.Generator().manual_seed(B + out + inp)
    ints = lambda *s: torch.randint(-8, 9, s, generator=g).to(F64)
    dy, x, w, db0, dx0 = ints(B, out), ints(B, inp), ints(out, inp), ints(1, out), ints(B, inp)
    assert 64 * out + 8 < R.LIMIT
    ady, ax, aw = place(dy, dtype=F32, mult=4, pad=4), place(x, dtype=BF16), place(w, dtype=BF16)
    adw, adb, adx = blank(out, inp, F32, ld=inp), place(db0, dtype=F32, mult=4, pad=4), place(dx0, dtype=F32, mult=4, pad=4)
    K.small_batch_linear_bwd(ady.view, ax.view, aw.view, adw.view, adb.view[0], adx.view)
    rep.equal("dW", adw.view, dy.t() @ x)
    rep.equal("db", adb.view[0], db0[0] + dy.sum(0))
    rep.equal("dX", adx.view, dx0 + dy @ w)
    rep.untouched("call", ady, ax, aw, adw, adb, adx)
    parts = blank(K.small_batch_linear_bwd_tiles(out) * B, inp, F32, ld=inp)
    K.small_batch_linear_bwd(ady.view, ax.view, aw.view, adw.view, None, dx_parts=parts.view.view(-1, B, inp))
    rep.equal("dX parts", parts.view.view(-1, B, inp).sum(0), dy @ w)      # (every part is a sum of integers: their fp32 sum is exact too)
    rep.equal("dW again", adw.view, dy.t() @ x)
    rep.untouched("dx_parts call", ady, ax, aw, adw, adb, adx, parts)
    rep.done()


# ------------------------------------------------------------------------------------------------ GELU: every bf16 pre-activation in [-100, 100]
def test_gelu_epilogue_exhaustive_sweep(K):
    """A = 0 and bias = every bf16 value in [-100, 100] (34 193 values along N, the last one repeated up to the tile): u = bf16(0 + bias) is that value.
    128 x 128 kernel and stagger 256 at M = 64, the persistent form at one tile row M = 256 over the sweep laid out twice (268 tiles > 256), the skinny
    GEMM at M = 8 with N = 34 193.  C and aux are finite and within the per-element bound of fp64 gelu / gelu'; aux is bit-identical between the three
    gemm_nt paths (they share gelu_tanh_both)."""
    u = R.all_bf16_between(-100.0, 100.0)
    n = u.numel()
    ay, ag = gelu_allowance()
    rep = Report("gelu sweep", (n,))
    auxes = {}

    def run(path, M, N, Kd, tile, skinny=False):
        vals = torch.cat([u, u])[:N] if N >= 2 * n else u
        vals = torch.cat([vals, vals[-1:].expand(N - vals.numel())]).float()
        u64 = vals.to(F64)[None, :]
        a = place(torch.zeros(M, Kd, dtype=BF16))
        b = place(torch.randint(-8, 9, (N, Kd), generator=torch.Generator().manual_seed(N)).to(BF16))
        bias, c = place(vals[None, :], mult=4, pad=4), blank(M, N, BF16)
        arenas = [a, b, bias, c]
        if skinny:
            K.gemm_skinny(a.view, b.view, out=c.view, epilogue=K.EPI_BIAS_GELU, bias=bias.view[0])
        else:
            aux = blank(M, N, BF16)
            arenas.append(aux)
            K.gemm_set_tile(tile)
            try:
                K.gemm_nt(a.view, b.view, out=c.view, epilogue=K.EPI_BIAS_GELU, bias=bias.view[0], aux=aux.view)
            finally:
                K.gemm_set_tile(-1)
            rep.gelu(f"{path} aux", aux.view, R.dgelu64(u64), ag)
            auxes[path] = aux.view[0, :n].clone()
            rep.equal(f"{path} aux rows identical", aux.view, aux.view[0:1].expand(M, N))
        rep.gelu(f"{path} C", c.view, R.gelu64(u64), ay)
        rep.untouched(path, *arenas)

    run("128x128", 64, up(n, 128), 128, 0)
    run("stagger 256", 64, up(n, 256), 128, 256)
    run("persistent 256", 256, 268 * 256, 128, 256)
    run("skinny", 8, n, 64, None, skinny=True)
    for path in ("stagger 256", "persistent 256"):
        rep.equal(f"aux of {path} = aux of 128x128", auxes[path].view(torch.int16), auxes["128x128"].view(torch.int16))
    rep.done()
