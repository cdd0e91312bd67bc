"""The row kernels of csrc/rowops.hip on a real MI355X (pytest -m gpu), from udm_norm_fwd to udm_qknorm_rope_bwd, through unidisc_amd.kernels: every output
against the fp64 restatement of tests/rowops_ref64.py, element by element, with the bounds derived there (never a whole-tensor ratio), on the input families
built to break a row kernel, out of NaN arenas.

Memory discipline.  Every floating-point operand and every caller-owned output is a view between NaN guard rows (gemm_ref64.arena); outputs that are
overwritten start as NaN (y, h, rstd, mean, stats, x_out, dx with accumulate = False, the q | k columns of d qkv - whose v columns must keep their NaN);
accumulated outputs (dx with accumulate = True, every column sum) start from a random tensor that the reference adds to; the wrappers' scratch is NaN before
every call; after it, everything outside the outputs is compared bit for bit.  (d branch of residual_bwd is allocated by the wrapper itself.)
The backward kernels take the statistics the forward kernels saved (checked against the reference first); the backward reference takes the same fp32 values.

Which parametrisation reaches which kernel, instance and grid is asserted on the CPU by tests/test_rowops_plan.py, which lists every call made here with the plan
csrc/rowops_plan.h gives it (B, L = 5, 37: ragged row chunks of one batch element and M % 4 != 0; M = 1, 3, 37: waves without a row and the ragged two-row group;
B, L = 2, 700: more rows than blocks; the other row counts: the first M past each grid cap and each workspace gate).
At M > 1024 the per-row outputs of the forward kernels are compared on a row sample (first, last, both sides of every grid seam); the backward reference runs
over all rows in chunks of 512 (the column sums need every row), so the per-row outputs of the backward kernels are compared on every row.
"""
import functools

import pytest
import torch

import gemm_ref64 as G
import ledger
import rowops_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "rowops_rowwise"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
GUARD = 16
SEAMS = (768, 1024, 1536, 2048, 3072, 4096, 8192)      # rows at which some grid of these kernels wraps around (blocks x rows per block)


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


@pytest.fixture(autouse=True)
def nan_scratch(K):
    """the wrappers' column-reduction scratch, sized beyond every shape here by one request, NaN before every test"""
    K._scratch(4096 * 4096, torch.empty(0, device=DEV).device).fill_(NAN)


class Mem:
    """the arenas of one case: inputs are checked for bit-identity after the calls, everything for untouched guards"""

    def __init__(self):
        self.arenas, self.inputs = [], []

    def _place(self, t, shape, ld):
        a = G.arena(shape, ld, t.dtype, guard_rows=GUARD, device=DEV, fill=t.reshape(shape))
        self.arenas.append(a)
        return a

    def inp(self, t):
        """a read-only operand"""
        if t is None:
            return None
        if not t.is_floating_point():
            return t.to(DEV)
        shape = tuple(t.shape) if t.dim() == 2 else (1, t.numel())
        a = self._place(t, shape, shape[1])
        self.inputs.append((a, t.reshape(shape).clone()))
        return a.view if t.dim() == 2 else a.view[0]

    def acc(self, t):
        """an accumulated output, starting from t"""
        shape = tuple(t.shape) if t.dim() == 2 else (1, t.numel())
        a = self._place(t, shape, shape[1])
        return a.view if t.dim() == 2 else a.view[0]

    def out(self, shape, dtype):
        """an overwritten output, starting as NaN"""
        s2 = tuple(shape) if len(shape) == 2 else (1, shape[0])
        a = G.arena(s2, s2[1], dtype, guard_rows=GUARD, device=DEV)
        self.arenas.append(a)
        return a.view if len(shape) == 2 else a.view[0]

    def check(self, what):
        for i, a in enumerate(self.arenas):
            G.assert_untouched(a, f"{what}: arena {i}")
        for a, t in self.inputs:
            assert torch.equal(a.view.cpu().view(G.INT_VIEW[a.dtype]), t.view(G.INT_VIEW[a.dtype])), f"{what}: an input operand changed"


def sample_windows(M):
    if M <= 1024:
        return [(0, M)]
    return [(0, 16)] + [(s - 8, s + 8) for s in SEAMS if 24 < s < M - 24] + [(M - 16, M)]


def chunks(M, n=512):
    return [(r, min(M, r + n)) for r in range(0, M, n)]


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def worst_ratios_to_the_ledger():
    yield
    for k, (r, note) in sorted(WORST.items()):
        ledger.record(TEST, k, r, 1.0, note=note)


class Tally:
    def __init__(self, name, family):
        self.name, self.family, self.worst = name, family, {}

    def rows(self, key, got, ref, E, r0=0):
        """got: the device rows [r0, r0 + n) of an output"""
        r, i = R.worst(got.cpu(), ref, E, key in R.BF16_OUT or key.split("/")[0] in R.BF16_OUT)
        if r > self.worst.get(key, (0.0, None))[0] or key not in self.worst:
            cols = ref.shape[-1] if ref.dim() > 1 else 1
            self.worst[key] = (r, (r0 + i // cols, i % cols))

    def done(self):
        bad = {k: v for k, v in self.worst.items() if not v[0] <= 1.0}
        for k, (r, where) in self.worst.items():          # the ledger keeps the worst ratio per kernel family, input family and output
            kk = f"{self.name.split('[')[0]}/{self.family}/{k}"
            if r >= WORST.get(kk, (-1.0,))[0]:
                WORST[kk] = (r, f"{self.name} at (row, col) = {where}")
        assert not bad, f"{self.name}: outside the bound (ratio, (row, col)): {bad}"


def fwd_rows(t, c, fwd_fn, got, keys):
    """the per-row outputs of a forward kernel against the reference on the sample windows; got: {key: device tensor with M rows}"""
    for r0, r1 in sample_windows(c.M):
        ref = fwd_fn(R.REF, R.window(c, r0, r1))
        for k in keys:
            t.rows(k, got[k][r0:r1], ref[k], ref["E_" + k], r0)
            if k + "_nr" in ref:
                t.rows(k + "/nr", got[k][r0:r1], ref[k + "_nr"], ref["E_" + k + "_nr"], r0)


def bwd_all(t, c, bwd_fn, stats, got_rows, got_cols, acc0, n_terms, window=R.window):
    """the backward reference over all rows in chunks: per-row outputs compared chunk by chunk, the column sums added up and compared at the end.
    stats: {name: device [M] / [M, 4]} saved by the forward kernel; acc0 / n_terms: {key: what the column sum started from / its number of terms}"""
    sums = {}
    for r0, r1 in chunks(c.M):
        ref = bwd_fn(R.REF, window(c, r0, r1), {k: v[r0:r1].cpu() for k, v in stats.items()}, prefill=False)
        for k, g in got_rows.items():
            t.rows(k, g[r0:r1], ref[k], ref["E_" + k], r0)
        for k in got_cols:
            for kk in (k, "E_" + k):
                sums[kk] = sums.get(kk, 0) + ref[kk]
    for k, g in got_cols.items():
        a0 = acc0[k].to(F64)
        t.rows(k, g, sums[k] + a0, sums["E_" + k] + (n_terms[k] + 8) * R.EF() * a0.abs())


def other_columns_unchanged(got, start, d, idx, what):
    """the columns of an adaLN gradient tensor outside the chunks `idx` keep their bits"""
    keep = torch.ones(start.shape[1], dtype=torch.bool)
    for k in idx:
        keep[k * d:(k + 1) * d] = False
    assert torch.equal(got.cpu()[:, keep].view(torch.int32), start[:, keep].view(torch.int32)), f"{what}: columns outside the written chunks changed"


# ------------------------------------------------------------------------------------------------ norm
def run_norm(K, c, accumulate=True):
    name = f"norm[{'rms' if c.nt == 0 else 'ln'},{c.mode},{c.family},M{c.M}(L{c.L}),d{c.d},acc{int(accumulate)}]"
    t, m = Tally(name, c.family), Mem()
    M, d = c.M, c.d
    x, w, dy, mod = m.inp(c.x), m.inp(c.w), m.inp(c.dy), m.inp(c.mod)
    modality, any_img = m.inp(c.modality), m.inp(c.any_img)
    y, rstd, mean = m.out((M, d), BF16), m.out((M,), F32), m.out((M,), F32) if c.nt else None
    K.norm_fwd(x, w, c.nt, c.L, mod=mod, mod_idx=R.MOD_IDX, modality=modality, any_img=any_img, out=(y, rstd, mean))
    got = dict(y=y, rstd=rstd, mean=mean)
    fwd_rows(t, c, R.norm_case_fwd, got, ("y", "rstd") + (("mean",) if c.nt else ()))
    dx = m.acc(c.dx0) if accumulate else m.out((M, d), F32)
    dw = m.acc(c.dw0)
    dmod = m.acc(c.dmod0) if c.mod is not None else None
    K.norm_bwd(dy, x, rstd, mean, w, c.nt, c.L, dx, dw, accumulate=accumulate, mod=mod, dmod=dmod, mod_idx=R.MOD_IDX, modality=modality, any_img=any_img)
    torch.cuda.synchronize()
    stats = dict(rstd=rstd, mean=mean if c.nt else torch.zeros(M, device=DEV))
    cols, acc0, n = dict(dw=dw), dict(dw=c.dw0), dict(dw=M)
    if c.mod is not None:
        for k, i in zip(("dshift", "dscale"), R.MOD_IDX):
            cols[k], acc0[k], n[k] = dmod[:c.B, i * d:(i + 1) * d], c.dmod0[:c.B, i * d:(i + 1) * d], c.L
        other_columns_unchanged(dmod, c.dmod0, d, R.MOD_IDX, name)
        assert torch.equal(dmod.cpu()[c.B:], c.dmod0[c.B:]), f"{name}: the padding rows of the adaLN gradient changed"
    bwd = functools.partial(R.norm_case_bwd, accumulate=accumulate)
    bwd_all(t, c, bwd, stats, dict(dx=dx), cols, acc0, n)
    m.check(name)
    t.done()


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_norm_families(K, family, d):
    """every template instance and its partial chunk on every family; B, L = 5, 37: ragged row chunks of one batch element, M % 4 != 0"""
    for nt in (0, 1):
        for mode in R.NORM_MODES:
            run_norm(K, R.norm_case(family, 5, 37, d, nt, mode))


NORM_ROWS = [
    (1, 1, 64, 0, "mod_all"), (1, 3, 768, 1, "plain"), (1, 37, 2048, 0, "mod_all"), (1, 1, 4096, 1, "plain"),
    (2, 700, 768, 0, "mod_img"), (2, 700, 2048, 1, "mod_all"),
    (1, 2048, 768, 0, "plain"), (1, 8200, 64, 1, "plain"), (2, 4100, 64, 0, "mod_img"),
    (1, 2051, 2048, 0, "plain"), (1, 2050, 4096, 1, "mod_all"),
]


@pytest.mark.parametrize("B,L,d,nt,mode", NORM_ROWS, ids=[f"b{b}_l{l}_d{d}_{'ln' if nt else 'rms'}_{mode}" for b, l, d, nt, mode in NORM_ROWS])
def test_norm_row_counts(K, B, L, d, nt, mode):
    """waves without a row, more rows than blocks, the workspace path of udm_norm_bwd, the first M past each grid cap (see the module docstring)"""
    run_norm(K, R.norm_case("gauss" if B * L < 4000 else "offset", B, L, d, nt, mode))


@pytest.mark.parametrize("d", [64, 1032, 2048])
def test_norm_bwd_overwrites_every_element_without_accumulate(K, d):
    for nt, mode in ((0, "plain"), (1, "mod_img")):
        run_norm(K, R.norm_case("gauss", 5, 37, d, nt, mode), accumulate=False)


# ------------------------------------------------------------------------------------------------ residual branch
def run_resid(K, c):
    name = f"residual[{c.variant},{c.family},M{c.M}(L{c.L}),d{c.d}]"
    t, m = Tally(name, c.family), Mem()
    M, d = c.M, c.d
    x_in, br, dxg = m.inp(c.x_in), m.inp(c.branch), m.inp(c.dx)
    w_b, w_n, mod, mod_n = m.inp(c.w_b), m.inp(c.w_n), m.inp(c.mod), m.inp(c.mod_n)
    modality, n_modality, n_any = m.inp(c.modality), m.inp(c.n_modality), m.inp(c.n_any_img)
    ln = c.nt == 1
    outs = (m.out((M, d), F32), m.out((M,), F32) if c.sandwich else None, m.out((M,), F32) if c.sandwich and ln else None,
            m.out((M, d), BF16) if c.nxt else None, m.out((M,), F32) if c.nxt else None, m.out((M,), F32) if c.nxt and ln else None)
    gate_idx = R.GATE_IDX if c.gate else None
    res = K.residual_fwd(x_in, br, c.L, w_b=w_b, norm_type=c.nt, mod=mod, gate_idx=gate_idx, modality=modality, p_drop=c.p, seed=R.SEED, next_w=w_n,
                         next_mod=mod_n, next_mod_idx=(0, 1), next_modality=n_modality, next_any_img=n_any, out=outs if c.nxt else outs[:3])
    x_out, rstd_b, mean_b = res[:3]
    got = dict(x_out=x_out, rstd_b=rstd_b, mean_b=mean_b)
    keys = ["x_out"] + (["rstd_b"] if c.sandwich else []) + (["mean_b"] if c.sandwich and ln else [])
    if c.nxt:
        got.update(h=res[3][0], rstd_n=res[3][1], mean_n=res[3][2])
        keys += ["h", "rstd_n"] + (["mean_n"] if ln else [])
    fwd_rows(t, c, R.resid_case_fwd, got, keys)
    if c.p > 0:          # the dropout mask itself: the elements the CPU Philox mask drops come out as x_in exactly, the kept ones (with a branch term that fp32 can see) do not
        for r0, r1 in sample_windows(M):
            keep = R.dropout_keep(R.SEED, c.p, r1 - r0, d, row0=r0)
            special = (torch.ones(r1 - r0, dtype=torch.bool) if c.modality is None else c.modality[r0:r1] == 1)[:, None].expand(r1 - r0, d)
            xi = c.x_in[r0:r1]
            ref = R.resid_case_fwd(R.REF, R.window(c, r0, r1))["x_out"]
            same = x_out[r0:r1].cpu() == xi
            assert bool(same[special & ~keep].all()), f"{name}: an element the CPU mask drops was kept, rows [{r0}, {r1})"
            seen = special & keep & ((ref - xi.double()).abs() > 2.0 ** -20 * xi.double().abs())
            assert not bool(same[seen].any()), f"{name}: an element the CPU mask keeps was dropped, rows [{r0}, {r1})"
    dw_b = m.acc(c.dw_b0) if c.sandwich else None
    dmod = m.acc(c.dmod0) if c.gate else None
    dbranch = K.residual_bwd(dxg, br, c.L, w_b=w_b, rstd=rstd_b, mean=mean_b, norm_type=c.nt, mod=mod, dmod=dmod, gate_idx=gate_idx, modality=modality, dw_b=dw_b,
                             p_drop=c.p, seed=R.SEED)
    torch.cuda.synchronize()
    stats = dict(rstd_b=rstd_b if c.sandwich else torch.zeros(M, device=DEV), mean_b=mean_b if c.sandwich and ln else torch.zeros(M, device=DEV))
    cols, acc0, n = {}, {}, {}
    if c.sandwich:
        cols["dw_b"], acc0["dw_b"], n["dw_b"] = dw_b, c.dw_b0, M
    if c.gate:
        i = R.GATE_IDX
        cols["dgate"], acc0["dgate"], n["dgate"] = dmod[:c.B, i * d:(i + 1) * d], c.dmod0[:c.B, i * d:(i + 1) * d], c.L
        other_columns_unchanged(dmod, c.dmod0, d, (i,), name)
        assert torch.equal(dmod.cpu()[c.B:], c.dmod0[c.B:]), f"{name}: the padding rows of the adaLN gradient changed"
    bwd_all(t, c, R.resid_case_bwd, stats, dict(dbranch=dbranch), cols, acc0, n)
    m.check(name)
    t.done()


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_residual_families(K, family, d):
    """every variant (sandwich rms / LayerNorm, gate on all rows / image rows, dropout, the fused next norm plain / modulated) on every family and width"""
    for variant in R.RESID_VARIANTS:
        run_resid(K, R.resid_case(family, 5, 37, d, variant))


RESID_ROWS = [
    (1, 1, 64, "sandwich_rms"), (1, 3, 2048, "gate_sandwich_dropout"), (1, 37, 4096, "sandwich_ln"), (1, 1, 3072, "gate_all"),
    (2, 700, 768, "gate_sandwich_dropout"), (2, 700, 2048, "gate_img_dropout"), (2, 700, 4096, "gate_sandwich_dropout"),
    (1, 8200, 64, "dropout"), (1, 8200, 64, "sandwich_rms"), (1, 4093, 768, "sandwich_rms"), (1, 4093, 768, "sandwich_ln"),
    (1, 2051, 2048, "sandwich_rms"), (1, 2051, 2048, "dropout"), (1, 2050, 4096, "sandwich_ln"),
]


@pytest.mark.parametrize("B,L,d,variant", RESID_ROWS, ids=[f"b{b}_l{l}_d{d}_{v}" for b, l, d, v in RESID_ROWS])
def test_residual_row_counts(K, B, L, d, variant):
    """waves without a row, more rows than blocks in the gated form, the wide-grid workspace form (M = 4093, d = 768), the first M past each grid cap"""
    run_resid(K, R.resid_case("gauss", B, L, d, variant))


# ------------------------------------------------------------------------------------------------ fused norm backward + residual-branch backward
def run_fused(K, c, ada, accumulate=True):
    name = f"fused{'_ada' if ada else ''}[{c.mode},{c.variant},{c.family},M{c.M}(L{c.L}),d{c.d},acc{int(accumulate)}]"
    t, m = Tally(name, c.family), Mem()
    n, r, M, d, z = c.n, c.r, c.M, c.d, torch.zeros(c.M, device=DEV)
    x, w, dy, br, w_b = m.inp(n.x), m.inp(n.w), m.inp(n.dy), m.inp(r.branch), m.inp(r.w_b)
    mod_n, mod_r, modality, any_img, modality_r = m.inp(n.mod), m.inp(r.mod), m.inp(n.modality), m.inp(n.any_img), m.inp(r.modality)
    _, rstd, mean = K.norm_fwd(x, w, c.nt, c.L)                     # the statistics the forward kernels save (held to the reference by the tests above)
    rstd_b = mean_b = None
    if r.sandwich:
        _, rstd_b, mean_b = K.residual_fwd(m.inp(r.x_in), br, c.L, w_b=w_b, norm_type=c.nt)
    dx = m.acc(n.dx0) if accumulate else m.out((M, d), F32)
    dbias0 = R._rn((d,), 77)
    # (where no fused form exists - d = 3072 - the wrapper runs the two kernels and `colsum`, whose transpose kernel refuses M % 8 != 0: no bias gradient there)
    dw, dbias = m.acc(n.dw0), m.acc(dbias0) if (d in (2048, 4096) or d < 2048 or M % 8 == 0) else None
    dw_b = m.acc(r.dw_b0) if r.sandwich else None
    dmod_n = m.acc(n.dmod0) if n.mod is not None else None
    dmod_r = m.acc(r.dmod0) if r.gate else None
    kw = dict(accumulate=accumulate, w_b=w_b, rstd_b=rstd_b, mean_b=mean_b, dw_b=dw_b, p_drop=r.p, seed=R.SEED, dbias=dbias)
    if ada:
        assert K.norm_residual_bwd_ada_ok(M, d, c.L)
        dbranch = K.norm_residual_bwd_ada(dy, x, rstd, mean, w, c.nt, c.L, dx, dw, br, mod_n=mod_n, dmod_n=dmod_n, mod_idx=R.MOD_IDX, modality=modality, any_img=any_img,
                                          mod_r=mod_r, dmod_r=dmod_r, gate_idx=R.GATE_IDX if r.gate else None, modality_r=modality_r, **kw)
    else:
        dbranch = K.norm_residual_bwd(dy, x, rstd, mean, w, c.nt, c.L, dx, dw, br, **kw)
    torch.cuda.synchronize()
    stats = dict(rstd=rstd, mean=mean if c.nt else z, rstd_b=rstd_b if r.sandwich else z, mean_b=mean_b if r.sandwich and c.nt else z)
    cols, acc0, nt_ = dict(dw=dw), dict(dw=n.dw0), dict(dw=M)
    if r.sandwich:
        cols["dw_b"], acc0["dw_b"], nt_["dw_b"] = dw_b, r.dw_b0, M
    if n.mod is not None:
        for k, i in zip(("dshift", "dscale"), R.MOD_IDX):
            cols[k], acc0[k], nt_[k] = dmod_n[:c.B, i * d:(i + 1) * d], n.dmod0[:c.B, i * d:(i + 1) * d], c.L
        other_columns_unchanged(dmod_n, n.dmod0, d, R.MOD_IDX, name)
    if r.gate:
        i = R.GATE_IDX
        cols["dgate"], acc0["dgate"], nt_["dgate"] = dmod_r[:c.B, i * d:(i + 1) * d], r.dmod0[:c.B, i * d:(i + 1) * d], c.L
        other_columns_unchanged(dmod_r, r.dmod0, d, (i,), name)
    bwd_all(t, c, functools.partial(R.fused_case_bwd, accumulate=accumulate), stats, dict(dx=dx, dbranch=dbranch), cols, acc0, nt_, window=R.fused_window)
    # the bias gradient: the column sums of the bf16 d branch the kernel itself wrote, in any order
    if dbias is not None:
        db = dbranch.double().cpu()
        t.rows("dbias", dbias, dbias0.double() + db.sum(0), (M + 8) * R.EF() * (dbias0.double().abs() + db.abs().sum(0)))
    m.check(name)
    t.done()


@pytest.mark.parametrize("d", R.WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_norm_residual_bwd_families(K, family, d):
    """udm_norm_residual_bwd: wave per row (d < 2048: NCH 1 .. 4), block per row (2048, 4096); d = 3072 runs the two separate kernels behind the same wrapper"""
    for variant in R.FUSED_VARIANTS:
        run_fused(K, R.fused_case(family, 5, 37, d, "plain", variant), ada=False)


@pytest.mark.parametrize("d", [2048, 4096])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_norm_residual_bwd_ada_families(K, family, d):
    """udm_norm_residual_bwd_ada: modulated norm (all rows / image rows) and / or gated branch (all rows / image rows), sandwich norm, dropout; one block per row"""
    for mode, variant in R.FUSED_ADA_VARIANTS.values():
        run_fused(K, R.fused_case(family, 5, 37, d, mode, variant), ada=True)


FUSED_ROWS = [
    (1, 1, 64, "plain", "sandwich_rms", False, True), (1, 3, 2048, "plain", "sandwich_ln", False, True), (1, 37, 768, "plain", "dropout", False, False),
    (1, 4100, 64, "plain", "sandwich_rms", False, True), (1, 1000, 2048, "plain", "sandwich_rms", False, True), (1, 1000, 4096, "plain", "sandwich_ln", False, False),
    (1, 1, 2048, "mod_all", "gate_all", True, True), (2, 700, 2048, "mod_img", "gate_sandwich_dropout", True, True), (2, 700, 4096, "mod_all", "sandwich_rms", True, False),
]


@pytest.mark.parametrize("B,L,d,mode,variant,ada,acc", FUSED_ROWS, ids=[f"b{b}_l{l}_d{d}_{mo}_{v}_acc{int(a)}" for b, l, d, mo, v, _, a in FUSED_ROWS])
def test_norm_residual_bwd_row_counts(K, B, L, d, mode, variant, ada, acc):
    """M = 4100 at d = 64: past the 1024-block cap of the wave-per-row form; M = 1000: past the 768 blocks of the block-per-row form; B, L = 2, 700: the adaLN
    form with more rows than blocks (bpb = 384); accumulate = False overwrites dx"""
    run_fused(K, R.fused_case("gauss", B, L, d, mode, variant), ada=ada, accumulate=acc)


# ------------------------------------------------------------------------------------------------ qk-norm + rotary
def run_qk(K, c, contiguous=True):
    name = f"qk[D{c.D},norm{int(c.qk_norm)},ps{int(c.per_sample)},qs{c.q_scale},{c.family},M{c.M}(L{c.L}),d{c.d},{'one' if contiguous else 'four'}]"
    t, m = Tally(name, c.family), Mem()
    M, d = c.M, c.d
    qkv, dqkr = m.inp(c.qkv), m.inp(c.dqkr)
    cos = m.inp(c.cos.reshape(-1, c.D // 2)).view(c.cos.shape)
    sin = m.inp(c.sin.reshape(-1, c.D // 2)).view(c.sin.shape)
    aff = {k: m.inp(v) for k, v in c.aff.items()}
    qkr, stats = m.out((M, 2 * d), BF16), m.out((M, 4), F32) if c.qk_norm else None
    K.qknorm_rope_fwd(qkv, cos, sin, c.L, c.D, q_scale=c.q_scale, out=(qkr, stats), **aff)
    fwd_rows(t, c, R.qk_case_fwd, dict(qkr=qkr, stats=stats), ("qkr",) + (("stats",) if c.qk_norm else ()))
    dqkv = m.out((M, 3 * d), BF16)
    names = ("dgq", "dbq", "dgk", "dbk")
    grads = {}
    if c.qk_norm:
        if contiguous:
            one = m.acc(torch.stack([c.acc0[k] for k in names]))
            grads = {k: one[i] for i, k in enumerate(names)}
        else:
            grads = {k: m.acc(c.acc0[k]) for k in names}
    K.qknorm_rope_bwd(dqkr, qkv, dqkv, cos, sin, c.L, c.D, gq=aff.get("gq"), gk=aff.get("gk"), stats=stats, q_scale=c.q_scale, **grads)
    torch.cuda.synchronize()
    v_cols = dqkv[:, 2 * d:].cpu().view(torch.int16)
    assert bool((v_cols == G.NAN_BITS[BF16]).all()), f"{name}: the v columns of d qkv were written"
    bwd_all(t, c, R.qk_case_bwd, dict(stats=stats) if c.qk_norm else dict(stats=torch.zeros(M, 4, device=DEV)), dict(dqk=dqkv[:, :2 * d]), grads,
            c.acc0 or {}, {k: M for k in names})
    m.check(name)
    t.done()


QK_WIDTHS = [d for d in R.WIDTHS if R.qk_heads(d)]


@pytest.mark.parametrize("d", QK_WIDTHS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_qknorm_rope_families(K, family, d):
    """D in {32, 64, 128, 256} wherever d % D == 0; the rope table by row % L and per sample; q_scale folded into q; qk-norm off (rotation only)"""
    for i, D in enumerate(R.qk_heads(d)):
        run_qk(K, R.qk_case(family, 5, 37, d, D, True, per_sample=bool(i & 1), q_scale=0.18 if i < 2 else 1.0), contiguous=bool(i & 1))
    run_qk(K, R.qk_case(family, 5, 37, d, R.qk_heads(d)[0], False, per_sample=False, q_scale=0.18))


QK_ROWS = [
    (1, 1, 64, 32, True), (1, 3, 2048, 128, True), (1, 37, 2048, 64, False), (1, 1, 4096, 256, True),
    (2, 700, 768, 64, True), (2, 700, 768, 64, False), (2, 700, 2048, 128, True), (2, 700, 2048, 128, False), (2, 700, 4096, 256, True),
    (2, 2050, 64, 32, True), (2, 2050, 64, 32, False), (1, 2051, 2048, 128, True), (1, 2050, 4096, 256, True), (1, 2050, 4096, 256, False),
]


@pytest.mark.parametrize("B,L,d,D,contiguous", QK_ROWS, ids=[f"b{b}_l{l}_d{d}_D{D}_{'one_alloc' if c else 'four_tensors'}" for b, l, d, D, c in QK_ROWS])
def test_qknorm_rope_row_counts(K, B, L, d, D, contiguous):
    """the ragged two-row group (odd M at d = 2048), the workspace and the atomics form of the backward, the first M past each grid cap"""
    run_qk(K, R.qk_case("gauss", B, L, d, D, True, per_sample=B * L == 37, q_scale=0.18), contiguous=contiguous)


# ------------------------------------------------------------------------------------------------ d > 4096
def test_wider_than_4096_is_refused(K):
    """the wave-per-row templates cover 4096 columns: d = 4104 is refused by the six entry points (rc 2, "unsupported hidden size") and nothing is written.
    The buffers have the full M x 4104 size."""
    M, d, L = 8, 4104, 8
    m = Mem()
    x, br, dy = m.inp(R._rn((M, d), 1)), m.inp(R._rn((M, d), 2).to(BF16)), m.inp(R._rn((M, d), 3).to(BF16))
    w, rstd = m.inp(1 + 0.1 * R._rn((d,), 4)), m.inp(torch.ones(M))
    mod = m.inp(R.mod_tensor(1, d, 6, 5))
    y, h, rs, rs2, xo = m.out((M, d), BF16), m.out((M, d), BF16), m.out((M,), F32), m.out((M,), F32), m.out((M, d), F32)
    dx, dw, dmod = m.out((M, d), F32), m.out((d,), F32), m.out((8, 6 * d), F32)
    calls = {
        "udm_norm_fwd": lambda: K.norm_fwd(x, w, 0, L, out=(y, rs, None)),
        "udm_norm_bwd": lambda: K.norm_bwd(dy, x, rstd, None, w, 0, L, dx, dw, accumulate=False),
        "udm_norm_bwd(modulated)": lambda: K.norm_bwd(dy, x, rstd, None, w, 0, L, dx, dw, accumulate=False, mod=mod, dmod=dmod),
        "udm_residual_fwd": lambda: K.residual_fwd(x, br, L, w_b=w, out=(xo, rs, None)),
        "udm_residual_norm_fwd": lambda: K.residual_fwd(x, br, L, next_w=w, out=(xo, None, None, h, rs2, None)),
        "udm_residual_norm_fwd_ada": lambda: K.residual_fwd(x, br, L, next_w=w, next_mod=mod, out=(xo, None, None, h, rs2, None)),
        "udm_residual_bwd": lambda: K.residual_bwd(x, br, L, w_b=w, rstd=rstd, dw_b=dw),
        "udm_residual_bwd(gated)": lambda: K.residual_bwd(x, br, L, mod=mod, dmod=dmod, gate_idx=5),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="unsupported hidden size"):
            call()
    torch.cuda.synchronize()
    for o in (y, h, rs, rs2, xo, dx, dw, dmod):
        assert bool(torch.isnan(o).all()), "a refused call wrote to its output"
    m.check("d = 4104")
