"""fp64 restatements of the row kernels (csrc/rowops.hip) and of the SUBS cross-entropy backward / full-row kernels (csrc/ce.hip), with per-element error
bounds, fp32 emulations, seeded mutants and adversarial input families (CPU only).

The reference of tests/test_gpu_rowops_rowwise.py and tests/test_gpu_ce_rowwise.py (GPU) and of tests/test_rowops_ref64.py (CPU); the split follows
attention_ref64.py / gemm_ref64.py.

One statement of every operation serves three purposes through an `Arith`: in fp64 with exact sums it is the reference; in fp32 with a chosen reduction order
and bf16 roundings at the kernels' rounding points it is an emulation (what a correct kernel may return); with a `mutant` it is a subtly wrong kernel the
comparator has to reject.  The GPU kernels are the independent implementation.

Rounding points, as the kernels document them
    norm_fwd            y = bf16(((x - mu) rs w) (1 + scale) + shift), statistics two-pass in fp32
    residual_fwd        n = (branch - mu) rs;  rms sandwich: n := bf16(n) (`.type_as(x)` of the reference RMSNorm on a bf16 input);  T = n w_b;  on "special" rows
                        (every row, or modality == 1) T := keep ? T ks : 0 with ks = fl32(1 / (1 - p)), then T := T gate;  x_out = x_in + T in fp32;
                        the fused next norm is norm_fwd on the fp32 x_out
    residual_bwd        n recomputed unrounded for the input gradient, bf16(n) (rms) in the dw_b / dgate terms; d branch rounded once to bf16
    qknorm_rope_fwd     a = bf16(LayerNorm(x) g + b) before the rotation; (a_lo cos - a_hi sin) q_scale rounded once to bf16 (q_scale on q only)
    qknorm_rope_bwd     no internal rounding (the normalised row is recomputed in fp32); d qkv rounded once to bf16
    subs_ce_bwd         d logits = bf16(g (onehot - exp(z - lse))) on the valid ids, 0 elsewhere

Error model.  u = 2^-8 (bf16), e = FACTOR 2^-24 (fp32, with the headroom factor), gamma = (d / 64 + 16) e: the deepest reduction tree of these kernels is
8 NCH = d / 64 sequential adds per lane, six butterfly steps and the cross-wave step (the block-per-row forms: d / 256 adds, the butterfly, a four-wave LDS pass).
A kernel with a deeper tree has to change `depth` knowingly.
Every output `name` comes with `E_name`, the fp32 part of its bound as an absolute error per element: gamma times the magnitude companion of every reduction
the element depends on (the same sum with each term replaced by its magnitude), plus e times the magnitudes of the element-wise products in front of it, one
per rounding (counted in the code), propagated through the statistics:
    mean      E_mu = gamma mean|x|                                       rstd      E_rs = (ms + eps - E_ms)^-1/2 - rs + 8 e rs
    variance  E_ms = gamma ms + 2 mean(|t| E_e) + mean((E_e + E_mu)^2)   (t = x - mu, E_e the element-wise part: the first-order effect of a shifted mean cancels,
                                                                          sum t = 0 - the property of the two-pass form that a one-pass E[x^2] - mu^2 does not have)
    input gradient of a norm, rs (G - mean G - xh mean(G xh)):  E = rs (gamma (mean|G| + |xh| mean|G xh|) + 12 e (|G| + mean|G| + |xh| mean|G xh|))
Classes of output and what `ratios` asserts, element by element:
    bf16, one rounding (y, h_out, d branch, d qkv, d logits)     |got - ref| <= u |ref| + (1 + u) E      (the rounding is relative to the fp32 value, up to |ref| + E)
    downstream of an internal bf16 rounding (rms sandwich: x_out, h_out, rstd_n; qk-norm: the rotated q | k)
         the rounded intermediate of a kernel lies between bf16(n - E_n) and bf16(n + E_n): `flip` = their distance is 0 except within E_n of a rounding
         boundary, where it is one bf16 spacing (in (u, 2u] |n|).  E carries flip times the magnitude the rounding scales (|w gate ks|, |cos| and |sin| times
         q_scale), so away from the boundaries these outputs are held to the fp32 bound.  The same outputs are ALSO compared with the statement without the
         internal rounding (`*_nr`), whose bound carries u times that magnitude on every element: u |n w gate ks|, u (|a_lo cos| + |a_hi sin|) q_scale.
    fp32 per row (rstd, mean, stats, x_out without the rms sandwich, dx)      |got - ref| <= E
    fp32 column sums (dw, dw_b, dshift, dscale, dgate, dgq, dbq, dgk, dbk)    any order of M terms (atomics):
         E = (M + 8) e sum_rows|term| + sum_rows E_term,  E_term = 8 e |term| (at most 8 roundings in any term) + flip parts;  |acc0| counts as a term.
         (M = L for the per-batch-element sums.)  The bias gradient of the fused backward is the column sum of the kernel's own bf16 d branch: (M + 8) e sum|d branch|.
    `ints` family: every partial sum of x and x^2 is exact in fp32 in any order, so the rms rstd and the LayerNorm mean get the d-independent 16 x 2^-24 relative
         (`exact_sums=True`, no headroom factor): a dropped or doubled element cannot hide under it.
    fused norm + residual backward: the residual half is linear in dx, so E_dx of the norm half is carried through it (`dx_err`).

FACTOR = 4.  tests/test_rowops_ref64.py measures, at factor 1 and with unrounded outputs, the worst ratio of the fp32 part that the two emulations reach on every
family at d = 64, 768, 1032, 4096 - the second emulation sums in the kernels' lane order and moves every rsqrt by +-2 ulp, which is where the device's rsqrtf may
differ from the CPU's.  Measured: 1.000 (x_out behind the rms sandwich and the plain x_out: a moved internal rounding meets its allowance of one bf16 spacing, a single fp32 add its
one counted rounding on a tie; rstd 0.50, dx 0.50, d qkv 0.69, d branch 0.59, column sums <= 0.17) -> the smallest power of two that leaves 4x headroom is 4.  CE_C = 8 the same way for d logits, E = CE_C 2^-23 ((1 + |z - lse|) p + [id == x0]) |g|
(+ 2^-126 max(|g|, 1): an exp below the fp32 normals may be flushed), the second emulation evaluating exp as exp2(fl(x log2 e)) moved by +-1 ulp: 1.30 at c = 1.
Quarter share: on every row of every family and width the fp32 part of a bf16 output's bound (without the flip allowances) is at most 1/4 of its bf16 part, the
worst being 0.20 (`offset`, d = 4096).  `offset_rows` as first drawn (ramp -32 .. 32) reached 0.39 at d = 4096 and is tamed to -16 .. 16.
"""
import math

import numpy as np
import torch

import attn_prob_dropout_ref as dropref

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -8
E32 = 2.0 ** -24
FACTOR = 4
CE_C = 8
TERM_ROUNDINGS = 8
NEG = -1000000.0
LSE_ATOL, LSE_RTOL = 2e-4, 1e-5          # the bound of tests/test_gpu_similarity_kernels.py::test_subs_logp_rows on lse

FAMILIES = ("gauss", "offset", "offset_rows", "huge", "tiny", "zero_rows", "spike_edges", "ints")
WIDTHS = (64, 520, 768, 1032, 2048, 3072, 4096)
CE_FAMILIES = ("gauss", "peaked", "flat", "forbidden_spikes", "large_negative")


def depth(d):
    """adds on the longest path of a row reduction (see the module docstring)"""
    return d / 64 + 16


_STATE = {"factor": FACTOR, "flips": True, "row0": 0, "M_total": None}


def gamma(d, factor=None):
    return (_STATE["factor"] if factor is None else factor) * depth(d) * E32


def EF():
    """the fp32 unit roundoff times the headroom factor: what one counted rounding is allowed"""
    return _STATE["factor"] * E32


def _factored(fn):
    """factor=... evaluates the bounds of one call at another headroom factor (the CPU test measures at factor 1); flips=False leaves the allowances for a
    moved internal bf16 rounding out of E (what remains is the fp32 part proper, the subject of the quarter-share condition); row0, M_total: the operands are rows
    [row0, row0 + M) of a problem of M_total rows (batch index, rope row and dropout counter follow the absolute row; the column sums are this window's share and
    their E is linear in the windows, so that the caller adds both up over the windows and adds acc0 with the first)"""
    def wrapped(*a, factor=None, flips=True, row0=0, M_total=None, **kw):
        old = dict(_STATE)
        _STATE.update(factor=old["factor"] if factor is None else factor, flips=flips and old["flips"], row0=row0, M_total=M_total)
        try:
            return fn(*a, **kw)
        finally:
            _STATE.update(old)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def eps_of(nt):
    return float(np.float32(1e-6 if nt == 0 else 1e-5))


def rbf(t):
    """round to bf16 (through fp32, as the kernels do), back in the dtype of t"""
    return t.to(F32).to(BF16).to(t.dtype)


def keep_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ input families
def make_rows(family, M, d, seed):
    """fp32 [M, d]"""
    g = torch.Generator().manual_seed(int(seed) * 7919 + 13 * M + d)
    n = torch.randn(M, d, generator=g)
    if family == "gauss":
        x = n * 2 + 0.3
    elif family == "offset":
        x = n + 16
    elif family == "offset_rows":
        x = n + torch.linspace(-16, 16, M)[:, None] if M > 1 else n + 16       # (-32 .. 32 fails the quarter-share condition at d >= 3072: tamed to 16)
    elif family == "huge":
        x = n * 3e4
    elif family == "tiny":
        x = n * 1e-3
    elif family == "zero_rows":
        x = n * 2 + 0.3
        x[::3] = 0
    elif family == "spike_edges":
        x = n * 0.01
        x[:, -1] += 100
        x[1::2, 0] -= 100
        if d > 512:
            x[:, 511] += 100
            x[:, 512] -= 100
    elif family == "ints":
        i = torch.randint(-8, 9, (M, d), generator=g).double()
        e = torch.randint(-6, 7, (M,), generator=g)
        x = torch.ldexp(i, e[:, None].expand(M, d))
    else:
        raise ValueError(family)
    return x.to(F32)


def ints_sums_exact(x):
    """every fp32 partial sum of x and of x^2 of an `ints` row is exact: the magnitudes sum below 2^24 units of the row's scale"""
    x = x.double()
    unit = x.abs().masked_fill(x == 0, float("inf")).min(-1).values
    unit = torch.where(torch.isinf(unit), torch.ones_like(unit), unit)
    k = x / unit[:, None]
    return bool((k == k.round()).all() and (k.abs().sum(-1) < 2 ** 24).all() and ((k * k).sum(-1) < 2 ** 24).all())


def mod_tensor(B, d, n, seed, scale=0.3):
    """bf16 [Bp, n d] adaLN output, rows past B zero (as the engine pads it)"""
    g = torch.Generator().manual_seed(int(seed) + 31 * d + B)
    Bp = (B + 7) // 8 * 8
    mod = torch.zeros(Bp, n * d)
    mod[:B] = torch.randn(B, n * d, generator=g) * scale
    return mod.to(BF16)


def chunk(mod, k, d, B):
    return None if mod is None else mod[:B, k * d:(k + 1) * d]


def dropout_keep(seed, p, M, d, row0=0):
    """bool [M, d]: the residual kernels' mask (dropout_keep8): element e = row d + col takes the 16-bit field e & 7 of philox4x32(seed, e >> 3), fields in the
    order x.lo x.hi y.lo y.hi z.lo z.hi w.lo w.hi; kept when field >= (uint32)(p 65536 + 0.5).  row0: the mask of rows [row0, row0 + M)."""
    assert d % 8 == 0
    thr = dropref.threshold(p)
    w = dropref.philox4x32(seed, np.arange(M * d // 8, dtype=np.uint64) + np.uint64(row0 * d // 8))
    f = np.stack([x for wd in w for x in (wd & np.uint64(0xFFFF), wd >> np.uint64(16))], -1)
    return torch.from_numpy((f >= thr).reshape(M, d))


# ------------------------------------------------------------------------------------------------ arithmetic
def _lane_sum(t):
    """the wave-per-row order: lane l adds its 8 columns of every 512-column chunk in turn, then a 64-lane butterfly"""
    M, d = t.shape
    nch = (d + 511) // 512
    v = torch.zeros(M, nch * 512, dtype=t.dtype)
    v[:, :d] = t
    v = v.view(M, nch, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, nch * 8)
    acc = torch.zeros(M, 64, dtype=t.dtype)
    for j in range(nch * 8):
        acc = acc + v[:, :, j]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, idx ^ o]
    return acc[:, 0]


class Arith:
    """dtype F64 + order 'exact': the reference.  dtype F32 + order 'torch' | 'lanes': an emulation (outputs rounded like the kernels').  mutant: see MUTANTS."""

    def __init__(self, dtype=F64, order="exact", rsqrt_ulps=0, mutant=None, round_out=True):
        self.dtype, self.order, self.rsqrt_ulps, self.mutant, self.round_out = dtype, order, rsqrt_ulps, mutant, round_out
        self.exact = dtype == F64

    def c(self, t):
        return None if t is None else t.to(self.dtype)

    def rowsum(self, t):
        if self.mutant == "drop_last8":
            t = t[:, :-8]
        return _lane_sum(t) if self.order == "lanes" else t.sum(-1)

    def div(self, d):
        return d - 8 if self.mutant == "mean_dm8" else d

    def rowsum_sum(self, t, groups, G=None):
        """sum over the rows of each group: t [M, d], groups int64 [M] in [0, G) or None (one group) -> [G, d] / [d]"""
        if self.order == "lanes":          # the opposite row order, one row at a time
            out = torch.zeros((G if groups is not None else 1, t.shape[1]), dtype=t.dtype)
            for r in range(t.shape[0] - 1, -1, -1):
                out[int(groups[r]) if groups is not None else 0] += t[r]
            return out if groups is not None else out[0]
        if groups is None:
            return t.sum(0)
        return torch.zeros(G, t.shape[1], dtype=t.dtype).index_add_(0, groups, t)

    def rsqrt(self, v):
        r = 1.0 / torch.sqrt(v)
        if self.rsqrt_ulps and not self.exact:
            k = torch.where(torch.arange(r.numel()) % 2 == 0, self.rsqrt_ulps, -self.rsqrt_ulps).to(torch.int32).reshape(r.shape)
            r = torch.where(torch.isfinite(r), (r.contiguous().view(torch.int32) + k).view(F32), r)
        return r

    def out_bf16(self, t):
        return t if self.exact or not self.round_out else t.to(BF16)


REF = Arith()
EMULATIONS = {"torch_order": Arith(F32, "torch"), "lane_order_rsqrt2ulp": Arith(F32, "lanes", rsqrt_ulps=2)}


def _rows(M):
    return torch.arange(M) + _STATE["row0"]


def _mtot(M):
    return _STATE["M_total"] or M


def _batch(ar, M, L):
    rows = _rows(M)
    if ar.mutant == "batch_seam":
        return torch.clamp((rows + 1) // L, max=(_mtot(M) - 1) // L)
    return rows // L


def _mod_rows(ar, M, shift, modality, any_img):
    if shift is None:
        return torch.zeros(M, dtype=torch.bool)
    img_only = modality is not None and (any_img is None or int(any_img) != 0)
    if not img_only or ar.mutant == "mod_text":
        return torch.ones(M, dtype=torch.bool)
    return modality == 1


def _stats(ar, v, nt, d):
    """two-pass statistics of the rows of v: mu, rs, t = v - mu, ms (mean square of t)"""
    dd = ar.div(d)
    if nt == 0:
        mu = torch.zeros(v.shape[0], dtype=v.dtype)
        t = v
        ms = ar.rowsum(v * v) / dd
    else:
        mu = ar.rowsum(v) / dd
        t = v - mu[:, None]
        ms = ar.rowsum(v * v) / dd - mu * mu if ar.mutant == "onepass_var" else ar.rowsum(t * t) / dd
    eps = 0.0 if ar.mutant == "no_eps" else eps_of(nt)
    return mu, ar.rsqrt(ms + eps), t, ms


def _stats_err(v, t, mu, rs, ms, nt, g, E_v=None, exact_sums=False):
    """(E_mu [M], E_rs [M], E_n [M, d]): bounds on the fp32 statistics and on n = t rs of rows whose elements carry the input error E_v (module docstring)"""
    E_v = torch.zeros_like(v) if E_v is None else E_v
    gs = 16 * E32 if exact_sums else g
    if nt == 0:
        E_mu = torch.zeros_like(mu)
        E_e = E_v
        g_ms = gs
    else:
        E_mu = E_v.mean(-1) + gs * v.abs().mean(-1)
        E_e = E_v + EF() * t.abs()
        g_ms = g
    E_ms = g_ms * ms + 2 * (t.abs() * E_e).mean(-1) + ((E_e + E_mu[:, None]) ** 2).mean(-1)
    eps = eps_of(nt)
    rs_hi = torch.clamp(ms + eps - E_ms, min=0.25 * eps) ** -0.5
    E_rs = (rs_hi - rs) + 8 * (E32 if exact_sums and nt == 0 else EF()) * rs
    E_t = E_e + E_mu[:, None]
    E_n = E_t * rs[:, None] + t.abs() * E_rs[:, None] + E_t * E_rs[:, None] + 2 * EF() * (t * rs[:, None]).abs()
    return E_mu, E_rs, E_n


def _flip(n, E_n):
    """distance between the bf16 roundings of the ends of [n - E_n, n + E_n]: 0 unless a rounding boundary lies inside"""
    return rbf(n + E_n) - rbf(n - E_n) if _STATE["flips"] else torch.zeros_like(n)


def _norm_apply(ar, n, w, shift, scale, mrow, b):
    """y = n w, modulated on the rows of mrow with the adaLN slices of batch element b[row]"""
    y = n * w
    if shift is not None:
        sc, sh = ar.c(scale)[b], ar.c(shift)[b]
        y = torch.where(mrow[:, None], y * (1 + sc) + sh, y)
    return y


def _norm_apply_err(n, E_n, w, shift, scale, mrow, b):
    aw = w.abs()
    mag = n.abs() * aw
    E = E_n * aw
    if shift is not None:
        sc, sh = scale.to(F64)[b].abs(), shift.to(F64)[b].abs()
        E = torch.where(mrow[:, None], E * (1 + sc), E)
        mag = torch.where(mrow[:, None], mag * (1 + sc) + sh, mag)
    return E + 4 * EF() * mag          # n w, 1 + scale, the product, + shift


# ------------------------------------------------------------------------------------------------ norm
@_factored
def norm_fwd(ar, x, w, nt, L, shift=None, scale=None, modality=None, any_img=None, exact_sums=False):
    """x fp32 [M, d], w fp32 [d], shift / scale bf16 [B, d] -> y, rstd, mean (+ E_*)"""
    M, d = x.shape
    x, w = ar.c(x), ar.c(w)
    mu, rs, t, ms = _stats(ar, x, nt, d)
    n = t * rs[:, None]
    b, mrow = _batch(ar, M, L), _mod_rows(ar, M, shift, modality, any_img)
    y = _norm_apply(ar, n, w, shift, scale, mrow, b)
    out = dict(y=ar.out_bf16(y), rstd=rs, mean=mu)
    if ar.exact:
        g = gamma(d)
        E_mu, E_rs, E_n = _stats_err(x, t, mu, rs, ms, nt, g, exact_sums=exact_sums)
        out.update(E_y=_norm_apply_err(n, E_n, w, shift, scale, mrow, b), E_rstd=E_rs, E_mean=E_mu)
    return out


def _norm_bwd_core(ar, G, A_G, xh, rs, nt, d, g):
    """rs (G - mean(G) - xh mean(G xh)) per row (the input gradient of a norm whose output gradient times weight is G); A_G: magnitude companion of G"""
    dd = ar.div(d)
    sgx = ar.rowsum(G * xh) / dd
    sg = ar.rowsum(G) / dd if nt else torch.zeros_like(sgx)
    o = rs[:, None] * (G - sg[:, None] - xh * sgx[:, None])
    if not ar.exact:
        return o, None
    A_sgx = (A_G * xh.abs()).mean(-1)
    A_sg = A_G.mean(-1) if nt else torch.zeros_like(A_sgx)
    mag = A_G + A_sg[:, None] + xh.abs() * A_sgx[:, None]
    E = rs[:, None] * (g * (A_sg[:, None] + xh.abs() * A_sgx[:, None]) + 12 * EF() * mag)
    return o, E


def _colsum_err(n, terms_abs, E_terms, acc0_abs):
    """any order of n terms: (n + 8) e sum|term| + the per-row bounds"""
    S = terms_abs + (0 if acc0_abs is None else acc0_abs)
    return (n + 8) * EF() * S + E_terms


@_factored
def norm_bwd(ar, dy, x, rstd, mean, w, nt, L, dx0=None, dw0=None, shift=None, scale=None, dshift0=None, dscale0=None, modality=None, any_img=None):
    """dy bf16, x fp32, rstd / mean fp32 [M] (inputs: the saved statistics) -> dx = dx0 + ..., dw = dw0 + ..., dshift / dscale [B, d] = ...0 + ... (+ E_*)"""
    M, d = x.shape
    B = (_mtot(M) + L - 1) // L
    dy, x, w, rs = ar.c(dy), ar.c(x), ar.c(w), ar.c(rstd)
    mu = ar.c(mean) if nt else torch.zeros(M, dtype=ar.dtype)
    b, mrow = _batch(ar, M, L), _mod_rows(ar, M, shift, modality, any_img)
    xh = (x - mu[:, None]) * rs[:, None]
    dyp = dy
    if shift is not None:
        dyp = torch.where(mrow[:, None], dy * (1 + ar.c(scale)[b]), dy)
    G = dyp * w
    g = gamma(d)
    o, E_o = _norm_bwd_core(ar, G, G.abs(), xh, rs, nt, d, g)
    dx = o if dx0 is None else ar.c(dx0) + o
    t_dw = dyp * xh
    dw = ar.rowsum_sum(t_dw, None) + (0 if dw0 is None else ar.c(dw0))
    out = dict(dx=dx, dw=dw)
    if shift is not None:
        zero = torch.zeros_like(dy)
        t_sh, t_sc = torch.where(mrow[:, None], dy, zero), torch.where(mrow[:, None], dy * xh * w, zero)
        out["dshift"] = ar.rowsum_sum(t_sh, b, B) + (0 if dshift0 is None else ar.c(dshift0))
        out["dscale"] = ar.rowsum_sum(t_sc, b, B) + (0 if dscale0 is None else ar.c(dscale0))
    if ar.exact:
        out["E_dx"] = E_o + EF() * (dx.abs() + (0 if dx0 is None else dx0.to(F64).abs()))
        a0 = lambda t: None if t is None else t.to(F64).abs()
        out["E_dw"] = _colsum_err(_mtot(M), t_dw.abs().sum(0), TERM_ROUNDINGS * EF() * t_dw.abs().sum(0), a0(dw0))
        if shift is not None:
            Lb = min(L, _mtot(M))
            for k, t_ in (("dshift", t_sh), ("dscale", t_sc)):
                S = torch.zeros(B, d, dtype=F64).index_add_(0, b, t_.abs())
                out["E_" + k] = _colsum_err(Lb, S, TERM_ROUNDINGS * EF() * S, a0(dshift0 if k == "dshift" else dscale0))
    return out


# ------------------------------------------------------------------------------------------------ residual branch
def _special(M, modality):
    return torch.ones(M, dtype=torch.bool) if modality is None else modality == 1


def _keep(ar, seed, p, M, d):
    if p <= 0:
        return None
    if ar.mutant == "dropout_ctr":           # the Philox counter shifted by one
        return dropout_keep(seed, p, M + 1, d, _STATE["row0"]).reshape(-1)[8:8 + M * d].reshape(M, d)
    return dropout_keep(seed, p, M, d, _STATE["row0"])


@_factored
def residual_fwd(ar, x_in, branch, L, w_b=None, nt=0, gate=None, modality=None, p_drop=0.0, seed=0, w_n=None, n_shift=None, n_scale=None, n_modality=None,
                 n_any_img=None, exact_sums=False):
    """x_in fp32 [M, d], branch bf16, w_b fp32 [d] (sandwich norm) or None, gate bf16 [B, d] or None -> x_out, rstd_b, mean_b and, with w_n, the fused next
    norm h, rstd_n, mean_n (+ E_*; with an rms sandwich also x_out_nr / E_x_out_nr, the statement without the internal rounding)"""
    M, d = x_in.shape
    x_in, br = ar.c(x_in), ar.c(branch)
    b, special = _batch(ar, M, L), _special(M, modality)
    g = gamma(d)
    out = {}
    E_T = E_Tnr = None
    if w_b is not None:
        wb = ar.c(w_b)
        mu, rs, t, ms = _stats(ar, br, nt, d)
        n = t * rs[:, None]
        out.update(rstd_b=rs, mean_b=mu)
        nr = rbf(n) if nt == 0 else n
        T, Tnr = nr * wb, n * wb
        if ar.exact:
            E_mu, E_rs, E_n = _stats_err(br, t, mu, rs, ms, nt, g, exact_sums=exact_sums)
            out.update(E_rstd_b=E_rs, E_mean_b=E_mu)
            E_T = (_flip(n, E_n) if nt == 0 else E_n) * wb.abs() + EF() * T.abs()
            E_Tnr = (E_n + U * n.abs()) * wb.abs() + EF() * Tnr.abs()
    else:
        T = Tnr = br
        if ar.exact:
            E_T = E_Tnr = torch.zeros_like(br)
    fac = torch.ones(M, d, dtype=ar.dtype)          # what the branch term is scaled by on special rows: keep ks gate
    keep = _keep(ar, seed, p_drop, M, d)
    nround = 0
    if keep is not None:
        fac = fac * keep.to(ar.dtype) * keep_scale(p_drop)
        nround += 1
    if gate is not None:
        fac = fac * ar.c(gate)[b]
        nround += 1
    fac = torch.where(special[:, None], fac, torch.ones_like(fac))
    if ar.exact:
        x_out = x_in + T * fac
        x_nr = x_in + Tnr * fac
        E_x = E_T * fac.abs() + (nround + 1) * EF() * (x_in.abs() + (T * fac).abs())
        E_xnr = E_Tnr * fac.abs() + (nround + 1) * EF() * (x_in.abs() + (Tnr * fac).abs())
        out.update(x_out=x_out, E_x_out=E_x)
        if w_b is not None and nt == 0:
            out.update(x_out_nr=x_nr, E_x_out_nr=E_xnr)
    else:                                            # the kernel's order of operations: dropout, then the gate, then the add
        o = T
        if keep is not None:
            o = torch.where(special[:, None], torch.where(keep, o * keep_scale(p_drop), torch.zeros_like(o)), o)
        if gate is not None:
            o = torch.where(special[:, None], o * ar.c(gate)[b], o)
        x_out = o + x_in
        out["x_out"] = x_out
    if w_n is not None:
        wn = ar.c(w_n)
        mu2, rs2, t2, ms2 = _stats(ar, x_out, nt, d)
        n2 = t2 * rs2[:, None]
        mrow = _mod_rows(ar, M, n_shift, n_modality, n_any_img)
        out.update(h=ar.out_bf16(_norm_apply(ar, n2, wn, n_shift, n_scale, mrow, b)), rstd_n=rs2, mean_n=mu2)
        if ar.exact:
            E_mu2, E_rs2, E_n2 = _stats_err(x_out, t2, mu2, rs2, ms2, nt, g, E_v=E_x, exact_sums=False)
            out.update(E_h=_norm_apply_err(n2, E_n2, wn, n_shift, n_scale, mrow, b), E_rstd_n=E_rs2, E_mean_n=E_mu2)
    return out


@_factored
def residual_bwd(ar, dx, branch, L, w_b=None, rstd_b=None, mean_b=None, nt=0, gate=None, modality=None, dw_b0=None, dgate0=None, p_drop=0.0, seed=0, dx_err=None):
    """dx fp32 [M, d] (grad wrt x_out), the saved branch and statistics -> dbranch (bf16), dw_b = dw_b0 + ..., dgate [B, d] = dgate0 + ... (+ E_*).
    dx_err: the error bound dx itself carries (the fused norm + residual backward hands its freshly computed dx on): every output is linear in dx"""
    M, d = dx.shape
    B = (_mtot(M) + L - 1) // L
    dn, br = ar.c(dx), ar.c(branch)
    E_dn = torch.zeros(M, d, dtype=F64) if dx_err is None else dx_err
    b, special = _batch(ar, M, L), _special(M, modality)
    g = gamma(d)
    keep = _keep(ar, seed, p_drop, M, d)
    dm = torch.ones(M, d, dtype=ar.dtype)
    if keep is not None:
        dm = torch.where(special[:, None], keep.to(ar.dtype) * keep_scale(p_drop), dm)
    out = {}
    flip = torch.zeros(M, d, dtype=F64)
    if w_b is not None:
        wb, rs = ar.c(w_b), ar.c(rstd_b)
        mu = ar.c(mean_b) if nt else torch.zeros(M, dtype=ar.dtype)
        nh = (br - mu[:, None]) * rs[:, None]
        nr = rbf(nh) if nt == 0 else nh
        if ar.exact and nt == 0:
            flip = _flip(nh, 2 * EF() * nh.abs())
        nn = nr * wb
    else:
        nn = br
    if gate is not None:
        gt = ar.c(gate)[b]
        zero = torch.zeros_like(dn)
        t_g = torch.where(special[:, None], dn * nn * dm, zero)
        out["dgate"] = ar.rowsum_sum(t_g, b, B) + (0 if dgate0 is None else ar.c(dgate0))
        if ar.exact:
            S = torch.zeros(B, d, dtype=F64).index_add_(0, b, t_g.abs())
            Ef = torch.zeros(B, d, dtype=F64).index_add_(0, b, torch.where(special[:, None], (dn * dm).abs() * flip * (wb.abs() if w_b is not None else 0)
                                                                           + E_dn * (nn * dm).abs(), zero))
            Lb = min(L, _mtot(M))
            out["E_dgate"] = _colsum_err(Lb, S, TERM_ROUNDINGS * EF() * S + Ef, None if dgate0 is None else dgate0.to(F64).abs())
        dn = torch.where(special[:, None], dn * gt, dn)
        E_dn = torch.where(special[:, None], E_dn * gt.abs().to(F64), E_dn)
    dn = dn * dm
    E_dn = E_dn * dm.abs().to(F64)
    if w_b is not None:
        t_w = dn * nr
        out["dw_b"] = ar.rowsum_sum(t_w, None) + (0 if dw_b0 is None else ar.c(dw_b0))
        o, E_o = _norm_bwd_core(ar, dn * wb, (dn * wb).abs(), nh, rs, nt, d, g)
        if ar.exact:
            E_G = E_dn * wb.abs()
            E_o = E_o + rs[:, None] * (E_G + (E_G.mean(-1) if nt else torch.zeros(M, dtype=F64))[:, None] + nh.abs() * (E_G * nh.abs()).mean(-1)[:, None])
            out["E_dw_b"] = _colsum_err(_mtot(M), t_w.abs().sum(0), TERM_ROUNDINGS * EF() * t_w.abs().sum(0) + (dn.abs() * flip + E_dn * nr.abs()).sum(0),
                                        None if dw_b0 is None else dw_b0.to(F64).abs())
    else:
        o, E_o = dn, 3 * EF() * dn.abs() + E_dn
    out["dbranch"] = ar.out_bf16(o)
    if ar.exact:
        out["E_dbranch"] = E_o
    return out


def norm_residual_bwd(ar, dy, x, rstd, mean, w, nt, L, branch, dx0=None, dw0=None, w_b=None, rstd_b=None, mean_b=None, dw_b0=None, p_drop=0.0, seed=0,
                      shift=None, scale=None, dshift0=None, dscale0=None, modality=None, any_img=None, gate=None, dgate0=None, modality_r=None, **win):
    """udm_norm_residual_bwd / udm_norm_residual_bwd_ada: the (modulated) norm backward, then the (gated) residual-branch backward at the UPDATED dx - the fp32 dx
    stays in registers between the two.  Outputs of both; the bias gradient (column sums of the bf16 d branch) is checked against the kernel's own d branch."""
    nb = norm_bwd(ar, dy, x, rstd, mean, w, nt, L, dx0=dx0, dw0=dw0, shift=shift, scale=scale, dshift0=dshift0, dscale0=dscale0, modality=modality,
                  any_img=any_img, **win)
    rb = residual_bwd(ar, nb["dx"] if ar.exact else nb["dx"].to(F32), branch, L, w_b=w_b, rstd_b=rstd_b, mean_b=mean_b, nt=nt, gate=gate, modality=modality_r,
                      dw_b0=dw_b0, dgate0=dgate0, p_drop=p_drop, seed=seed, dx_err=nb.get("E_dx"), **win)
    return dict(nb, **rb)


# ------------------------------------------------------------------------------------------------ qk-norm + rotary
def _halves(D, d):
    """column indices of the lower and the upper half of every head"""
    c = torch.arange(d)
    return c[(c % D) < D // 2], c[(c % D) >= D // 2]


def _rope_rows(ar, M, L, cos):
    r = _rows(M)
    if cos.dim() == 3:
        return r
    if ar.mutant == "rope_row":      # the table read at `row`: past its L rows from the second batch element on (restated as the neighbouring row of the table)
        return torch.where(r < L, r, (r + 1) % L)
    return r % L


@_factored
def qknorm_rope_fwd(ar, qkv, cos, sin, L, D, gq=None, bq=None, gk=None, bk=None, q_scale=1.0, exact_sums=False):
    """qkv bf16 [M, 3 d], cos / sin fp32 [L, D / 2] (indexed by row % L) or [B, L, D / 2] (by row) -> qkr [M, 2 d] (bf16), stats [M, 4] (+ E_*, qkr_nr)"""
    M, d = qkv.shape[0], qkv.shape[1] // 3
    H = d // D
    lo, hi = _halves(D, d)
    tr = _rope_rows(ar, M, L, cos)
    cs = ar.c(cos.reshape(-1, D // 2))[tr].repeat(1, H)           # [M, d / 2]: the table repeats per head
    sn = ar.c(sin.reshape(-1, D // 2))[tr].repeat(1, H)
    if ar.mutant == "rot_sign":
        sn = -sn
    qs = float(np.float32(q_scale))
    g = gamma(d)
    outs, outs_nr, Es, Es_nr, stats, E_stats = [], [], [], [], [], []
    for part, (ga, be) in enumerate(((gq, bq), (gk, bk))):
        x = ar.c(qkv[:, part * d:(part + 1) * d])
        s = qs if (part == 0) != (ar.mutant == "qscale_on_k") else 1.0
        flip = E_a = None
        if ga is not None:
            mu, rs, t, ms = _stats(ar, x, 1, d)
            n = t * rs[:, None]
            a_nr = n * ar.c(ga) + ar.c(be)
            a = rbf(a_nr)
            stats += [mu, rs]
            if ar.exact:
                E_mu, E_rs, E_n = _stats_err(x, t, mu, rs, ms, 1, g, exact_sums=exact_sums)
                E_a = E_n * ga.to(F64).abs() + 2 * EF() * ((n * ga.to(F64)).abs() + be.to(F64).abs())
                flip = _flip(a_nr, E_a)
                E_stats += [E_mu, E_rs]
        else:
            a = a_nr = x
        al, ah = a[:, lo], a[:, hi]
        o = torch.empty_like(a)
        o[:, lo] = (al * cs - ah * sn) * s
        o[:, hi] = (ah * cs + al * sn) * s
        outs.append(ar.out_bf16(o))
        if ar.exact:
            A = torch.empty_like(a)
            A[:, lo] = (al * cs).abs() + (ah * sn).abs()
            A[:, hi] = (ah * cs).abs() + (al * sn).abs()
            E = 4 * EF() * A * s
            E_nr = E
            if ga is not None:
                F_, Fn = torch.empty_like(a), torch.empty_like(a)
                F_[:, lo] = flip[:, lo] * cs.abs() + flip[:, hi] * sn.abs()
                F_[:, hi] = flip[:, hi] * cs.abs() + flip[:, lo] * sn.abs()
                Fn[:, lo] = E_a[:, lo] * cs.abs() + E_a[:, hi] * sn.abs()
                Fn[:, hi] = E_a[:, hi] * cs.abs() + E_a[:, lo] * sn.abs()
                anl, anh = a_nr[:, lo], a_nr[:, hi]
                onr, Anr = torch.empty_like(a), torch.empty_like(a)
                onr[:, lo] = (anl * cs - anh * sn) * s
                onr[:, hi] = (anh * cs + anl * sn) * s
                Anr[:, lo] = (anl * cs).abs() + (anh * sn).abs()
                Anr[:, hi] = (anh * cs).abs() + (anl * sn).abs()
                outs_nr.append(onr)
                Es_nr.append((Fn + U * Anr + 4 * EF() * Anr) * s)
                E = E + F_ * s
            Es.append(E)
    out = dict(qkr=torch.cat(outs, 1))
    if gq is not None:
        out["stats"] = torch.stack(stats, 1)
    if ar.exact:
        out["E_qkr"] = torch.cat(Es, 1)
        if gq is not None:
            out.update(E_stats=torch.stack(E_stats, 1), qkr_nr=torch.cat(outs_nr, 1), E_qkr_nr=torch.cat(Es_nr, 1))
    return out


@_factored
def qknorm_rope_bwd(ar, dqkr, qkv, cos, sin, L, D, gq=None, gk=None, stats=None, acc0=None, q_scale=1.0):
    """dqkr bf16 [M, 2 d], the saved qkv and stats (fp32 [M, 4], inputs) -> dqk [M, 2 d] (bf16: columns [0, 2 d) of d qkv), dgq dbq dgk dbk = acc0[...] + ..."""
    M, d = qkv.shape[0], qkv.shape[1] // 3
    H = d // D
    lo, hi = _halves(D, d)
    tr = _rope_rows(ar, M, L, cos)
    cs = ar.c(cos.reshape(-1, D // 2))[tr].repeat(1, H)
    sn = ar.c(sin.reshape(-1, D // 2))[tr].repeat(1, H)
    if ar.mutant == "rot_sign":
        sn = -sn
    qs = float(np.float32(q_scale))
    g = gamma(d)
    outs, Es, out = [], [], {}
    for part, ga in enumerate((gq, gk)):
        dz = ar.c(dqkr[:, part * d:(part + 1) * d])
        if (part == 0) != (ar.mutant == "qscale_on_k"):
            dz = dz * qs
        dl, dh = dz[:, lo], dz[:, hi]
        G0, A0 = torch.empty_like(dz), torch.empty_like(dz)
        G0[:, lo] = dl * cs + dh * sn
        G0[:, hi] = dh * cs - dl * sn
        A0[:, lo] = (dl * cs).abs() + (dh * sn).abs()
        A0[:, hi] = (dh * cs).abs() + (dl * sn).abs()
        if ga is None:
            outs.append(ar.out_bf16(G0))
            Es.append(4 * EF() * A0)
            continue
        x = ar.c(qkv[:, part * d:(part + 1) * d])
        mu, rs = ar.c(stats[:, 2 * part]), ar.c(stats[:, 2 * part + 1])
        xh = (x - mu[:, None]) * rs[:, None]
        gg = ar.c(ga)
        o, E_o = _norm_bwd_core(ar, G0 * gg, A0 * gg.abs(), xh, rs, 1, d, g)
        outs.append(ar.out_bf16(o))
        names = ("dgq", "dbq") if part == 0 else ("dgk", "dbk")
        for nm, t_, A_ in ((names[0], G0 * xh, A0 * xh.abs()), (names[1], G0, A0)):
            a0 = None if acc0 is None else acc0[nm]
            out[nm] = ar.rowsum_sum(t_, None) + (0 if a0 is None else ar.c(a0))
            if ar.exact:
                S = A_.sum(0)
                out["E_" + nm] = _colsum_err(_mtot(M), S, TERM_ROUNDINGS * EF() * S, None if a0 is None else a0.to(F64).abs())
        if ar.exact:
            Es.append(E_o)
    out["dqk"] = torch.cat(outs, 1)
    if ar.exact:
        out["E_dqk"] = torch.cat(Es, 1)
    return out


# ------------------------------------------------------------------------------------------------ comparison
def ratios(got, ref, E, bf16):
    """|got - ref| / (u |ref| [bf16 outputs] + E) per element; 0 where both vanish, inf where got is not finite or a zero bound is missed"""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).abs()
    bound = (U * ref.abs() + (1 + U) * E) if bf16 else E          # the output rounding is relative to the fp32 value the kernel holds, up to |ref| + E
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))


def worst(got, ref, E, bf16):
    """(largest ratio, its index)"""
    r = ratios(got, ref, E, bf16).reshape(-1)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return float(r[i]), i


def quarter_share(ref, E):
    """largest over the rows of (sum of the fp32 part E) / (sum of the bf16 part u |ref|): the condition asks <= 1 / 4 (rows that are exactly zero: 0)"""
    a, b = E.sum(-1), (U * ref.abs()).sum(-1)
    return float(torch.where(a == 0, torch.zeros_like(a), a / b).max())


BF16_OUT = {"y", "h", "dbranch", "qkr", "qkr_nr", "dqk"}


def compare(got, ref, keys=None):
    """{key: (worst ratio, flat index)} over the outputs of `ref` that `got` holds"""
    res = {}
    for k in (keys or [k for k in ref if not k.startswith("E_") and k in got and got[k] is not None]):
        res[k] = worst(got[k], ref[k], ref["E_" + k], k in BF16_OUT)
    return res


# ------------------------------------------------------------------------------------------------ SUBS cross-entropy
def valid_ids(M, V, Vt, mask_id, modality, restrict, mutant=None):
    """bool [M, V]: [lo, hi) minus mask_id (valid_range of csrc/ce.hip)"""
    ar = torch.arange(V)[None]
    seam = Vt + 1 if mutant == "seam_off_by_one" else Vt
    v = torch.ones(M, V, dtype=torch.bool)
    if restrict:
        v = torch.where((modality == 1)[:, None], ar >= seam, ar < seam).clone()
    if mutant != "mask_id_admitted":
        v[:, mask_id] = False
    return v


def ce_case(family, V, Vt, mask_id, M=48, ld=None, seed=0):
    """logits bf16 [M, ld] (finite everywhere), x0, xt, modality, g, ld.  Even rows are [MASK] rows, odd rows unmasked; rows 2, 3 mod 4 are image rows when the
    vocabulary has an image part.  Every family keeps: g == 0 on a masked row (4); x0 = mask_id, the NEG branch (6); x0 at the first valid id of the row's
    range (8, 10), at the last (12, 14), next to mask_id (16 .. 22: on rows of the other modality that is an invalid x0 under the restriction)."""
    g_ = torch.Generator().manual_seed(9000 + V + 17 * seed + CE_FAMILIES.index(family))
    ld = ld or (V + 127) // 128 * 128
    two = V > Vt
    modality = (torch.arange(M) % 4 >= 2).long() if two else torch.zeros(M, dtype=torch.long)
    img = modality == 1
    z = torch.zeros(M, ld)
    base = torch.randn(M, V, generator=g_) * 2.0
    x0 = torch.where(img, torch.randint(Vt, max(V, Vt + 1), (M,), generator=g_), torch.randint(0, Vt, (M,), generator=g_))
    lo, hi = torch.where(img, Vt, 0), torch.where(img, V, Vt)          # the row's own modality range
    for r in range(M):                                                  # keep the random x0 valid
        while int(x0[r]) == mask_id:
            x0[r] = int(lo[r]) + (int(x0[r]) - int(lo[r]) + 1) % int(hi[r] - lo[r])
    first = [int(lo[r]) + (1 if int(lo[r]) == mask_id else 0) for r in range(M)]
    last = [int(hi[r]) - 1 - (1 if int(hi[r]) - 1 == mask_id else 0) for r in range(M)]
    near = mask_id + 1 if mask_id + 1 < V and mask_id + 1 != Vt else mask_id - 1
    for r in (8, 10):
        x0[r] = first[r]
    for r in (12, 14):
        x0[r] = last[r]
    for r in (16, 18, 20, 22):                                          # next to mask_id, on rows of the modality that owns it (and on the others: invalid under restrict)
        x0[r] = near
    x0[6] = mask_id
    if family == "gauss":
        z[:, :V] = base
    elif family == "peaked":
        z[:, :V] = base
        for r in range(M):
            on = r % 8 < 4 and int(x0[r]) != mask_id and int(lo[r]) <= int(x0[r]) < int(hi[r])       # x0 on the peak / off it
            pk = int(x0[r]) if on else first[r] + (2 if first[r] + 2 != mask_id else 3)
            z[r, pk] += 60.0
    elif family == "flat":
        z[:, :V] = 1.25
    elif family == "forbidden_spikes":
        z[:, :V] = base
        z[:, mask_id] += 80.0
        z[:, Vt - 1] += 80.0
        if two:
            z[:, Vt] += 80.0
        for r in range(M):
            z[r, last[r]] += 80.0
    elif family == "large_negative":
        z[:, :V] = base - 300.0
    else:
        raise ValueError(family)
    xt = x0.clone()
    xt[::2] = mask_id
    g = torch.randn(M, generator=g_)
    g[4] = 0.0
    return z.to(BF16), x0, xt, modality, g.to(F32), ld


def ce_poison(z, valid, V):
    """NaN in every column the kernels must not depend on: [V, ld) and the ids outside `valid`"""
    p = z.clone()
    p[:, V:] = float("nan")
    p[:, :V] = torch.where(valid, p[:, :V], torch.full_like(p[:, :V], float("nan")))
    return p


def lse64(z, valid, V):
    return torch.logsumexp(z[:, :V].double().masked_fill(~valid, float("-inf")), -1)


def subs_ce_fwd64(z, x0, xt, valid, V, mask_id):
    """(log_p, lse) fp64: unmasked rows 0 / NEG and lse 0; masked rows z[x0] - lse with z[x0] := NEG for an invalid x0"""
    lse = lse64(z, valid, V)
    masked = xt == mask_id
    ok = valid.gather(1, x0.clamp(0, V - 1)[:, None])[:, 0] & (x0 >= 0) & (x0 < V)
    zx = torch.where(ok, z[:, :V].double().gather(1, x0.clamp(0, V - 1)[:, None])[:, 0], torch.full((z.shape[0],), NEG, dtype=F64))
    lp = torch.where(masked, zx - lse, torch.where(x0 == xt, 0.0, NEG).double())
    return lp, torch.where(masked, lse, torch.zeros_like(lse))


def _exp(ar, a, fast):
    if not fast:
        return torch.exp(a)
    e = torch.exp2((a * float(np.float32(1.4426950408889634))).to(F32).double()).to(F32)      # exp2 of the ROUNDED product, correctly rounded
    k = torch.where(torch.arange(e.numel()) % 2 == 0, 1, -1).to(torch.int32).reshape(e.shape)
    return torch.where(e > 0, (e.contiguous().view(torch.int32) + k).view(F32), e)


def subs_ce_bwd(ar, z, x0, xt, lse, g, valid, V, mask_id, window=None, sentinel=None, fast_exp=False, c=None):
    """d logits [M, ld]: g (onehot(x0) - exp(z - lse)) on the valid ids of the masked rows with g != 0, 0 on every other column of the written window;
    window: bool [M, ld] (the narrow form) - outside it the buffer keeps `sentinel`.  lse, g: fp32 inputs.  (+ E_dlogits)"""
    M, ld = z.shape
    zz = ar.c(z[:, :V])
    act = ((xt == mask_id) & (g != 0))[:, None] & valid
    a = torch.where(act, zz - ar.c(lse)[:, None], torch.zeros_like(zz))
    p = torch.where(act, _exp(ar, a, fast_exp), torch.zeros_like(zz))
    onehot = torch.zeros(M, V, dtype=ar.dtype).scatter_(1, x0.clamp(0, V - 1)[:, None], 1.0)
    dl = torch.zeros(M, ld, dtype=ar.dtype)
    dl[:, :V] = torch.where(act, ar.c(g)[:, None] * (onehot - p), torch.zeros_like(zz))
    out = dict(dlogits=ar.out_bf16(dl))
    if ar.exact:
        E = torch.zeros(M, ld, dtype=F64)
        cc = CE_C if c is None else c
        E[:, :V] = cc * 2.0 ** -23 * ((1 + a.abs()) * p + torch.where(act, onehot, torch.zeros_like(p))) * g.double().abs()[:, None]   # at x0: 1 - p and the product round relative to |g|
        E[:, :V] += torch.where(act, 2.0 ** -126 * g.double().abs().clamp(min=1.0)[:, None], torch.zeros_like(p))   # an exp below the fp32 normals may be flushed
        out["E_dlogits"] = E
    if window is not None:
        for k in list(out):
            out[k] = torch.where(window, out[k], sentinel.to(out[k].dtype) if k == "dlogits" else torch.zeros_like(out[k]))
    return out


def narrow_window(M, ld, Vt, n_txt):
    """bool [M, ld]: what udm_subs_ce_bwd writes with narrow_txt_rows = n_txt: rows [0, n) columns [0, ceil64(Vt)), the rest [floor8(Vt), ld)"""
    c = torch.arange(ld)[None]
    r = torch.arange(M)[:, None]
    return torch.where(r < n_txt, c < min((Vt + 63) // 64 * 64, ld), c >= Vt // 8 * 8)


def subs_logprobs64(z, xt, valid, V, mask_id):
    """fp64 [M, V]: masked rows z - lse on the valid ids, NEG elsewhere; unmasked rows 0 at xt, NEG elsewhere"""
    lse = lse64(z, valid, V)
    m = torch.where(valid, z[:, :V].double() - lse[:, None], torch.full((1,), NEG, dtype=F64))
    um = torch.full_like(m, NEG).scatter_(1, xt.clamp(0, V - 1)[:, None], 0.0)
    return torch.where((xt == mask_id)[:, None], m, um)


MUTANTS = ("drop_last8", "mean_dm8", "onepass_var", "no_eps", "mod_text", "batch_seam", "dropout_ctr", "rope_row", "rot_sign", "qscale_on_k",
           "mask_id_admitted", "seam_off_by_one", "assign_not_accumulate")


# ------------------------------------------------------------------------------------------------ cases shared by the CPU and the GPU tests
import types

NORM_MODES = ("plain", "mod_all", "mod_img")
# residual variants: sandwich norm, its type, gate, gate / dropout on image rows only, dropout p, the fused next norm ("" none, "plain", "mod_all", "mod_img")
RESID_VARIANTS = {
    "plain": dict(sandwich=False, nt=0, gate=False, img=False, p=0.0, nxt="plain"),
    "sandwich_rms": dict(sandwich=True, nt=0, gate=False, img=False, p=0.0, nxt="mod_img"),
    "sandwich_ln": dict(sandwich=True, nt=1, gate=False, img=False, p=0.0, nxt="plain"),
    "gate_all": dict(sandwich=False, nt=0, gate=True, img=False, p=0.0, nxt="mod_all"),
    "gate_img_dropout": dict(sandwich=False, nt=1, gate=True, img=True, p=0.1, nxt="mod_img"),
    "gate_sandwich_dropout": dict(sandwich=True, nt=0, gate=True, img=False, p=0.1, nxt=""),
    "dropout": dict(sandwich=False, nt=0, gate=False, img=False, p=0.25, nxt="plain"),
}
MOD_IDX, GATE_IDX, SEED = (3, 4), 5, 0x5EED0123456789


def _rn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed))) * scale


def _modality(M, L, frac=2):
    return (torch.arange(M) % L >= L // frac).long()


def norm_case(family, B, L, d, nt, mode, seed=1):
    M = B * L
    c = types.SimpleNamespace(M=M, B=B, L=L, d=d, nt=nt, mode=mode, family=family)
    c.x, c.w = make_rows(family, M, d, seed), 1 + 0.1 * _rn((d,), seed + 1)
    c.dy, c.dx0, c.dw0 = _rn((M, d), seed + 2).to(BF16), _rn((M, d), seed + 3), _rn((d,), seed + 4)
    c.mod = mod_tensor(B, d, 6, seed + 5) if mode != "plain" else None
    c.dmod0 = _rn(tuple(c.mod.shape), seed + 6) if c.mod is not None else None
    c.modality = _modality(M, L) if mode == "mod_img" else None
    c.any_img = torch.ones(1, dtype=torch.int32) if mode == "mod_img" else None
    c.kw = dict(shift=chunk(c.mod, MOD_IDX[0], d, B), scale=chunk(c.mod, MOD_IDX[1], d, B), modality=c.modality, any_img=c.any_img)
    c.exact_sums = family == "ints"
    return c


ROW_ATTRS = ("x", "dy", "dx0", "modality", "x_in", "branch", "dx", "n_modality", "qkv", "dqkr")


def window(c, r0, r1):
    """rows [r0, r1) of a case: the reference then runs on them alone (see `_factored`)"""
    w = types.SimpleNamespace(**vars(c))
    for a in ROW_ATTRS:
        if getattr(c, a, None) is not None:
            setattr(w, a, getattr(c, a)[r0:r1])
    w.row0, w.M_total, w.M = r0 + getattr(c, "row0", 0), getattr(c, "M_total", None) or c.M, r1 - r0
    if hasattr(c, "kw"):
        w.kw = dict(c.kw, modality=w.modality)
    return w


def _win(c):
    return dict(row0=getattr(c, "row0", 0), M_total=getattr(c, "M_total", None))


def norm_case_fwd(ar, c, factor=None, flips=True):
    return norm_fwd(ar, c.x, c.w, c.nt, c.L, factor=factor, flips=flips, exact_sums=c.exact_sums, **c.kw, **_win(c))


def norm_case_bwd(ar, c, fwd, factor=None, accumulate=True, prefill=True):
    """fwd: the fp64 forward of the case - its statistics, rounded to fp32, are the saved inputs of the backward"""
    kw = dict(c.kw)
    if c.mod is not None and prefill:
        kw.update(dshift0=chunk(c.dmod0, MOD_IDX[0], c.d, c.B), dscale0=chunk(c.dmod0, MOD_IDX[1], c.d, c.B))
    return norm_bwd(ar, c.dy, c.x, fwd["rstd"].to(F32), fwd["mean"].to(F32), c.w, c.nt, c.L, dx0=c.dx0 if accumulate else None,
                    dw0=c.dw0 if prefill else None, factor=factor, **kw, **_win(c))


def resid_case(family, B, L, d, variant, seed=2):
    v = RESID_VARIANTS[variant]
    M = B * L
    c = types.SimpleNamespace(M=M, B=B, L=L, d=d, variant=variant, family=family, **v)
    c.x_in, c.branch, c.dx = _rn((M, d), seed), make_rows(family, M, d, seed + 1).to(BF16), _rn((M, d), seed + 2)
    c.w_b = 1 + 0.1 * _rn((d,), seed + 3) if c.sandwich else None
    c.w_n = 1 + 0.1 * _rn((d,), seed + 4) if c.nxt else None
    c.mod = mod_tensor(B, d, 6, seed + 5) if c.gate else None
    c.mod_n = mod_tensor(B, d, 2, seed + 6) if c.nxt.startswith("mod") else None       # the next norm's adaLN tensor has its own row stride
    c.modality = _modality(M, L, 3) if c.img else None
    c.n_modality = _modality(M, L) if c.nxt == "mod_img" else None
    c.n_any_img = torch.ones(1, dtype=torch.int32) if c.nxt == "mod_img" else None
    c.dw_b0 = _rn((d,), seed + 7) if c.sandwich else None
    c.dmod0 = _rn(tuple(c.mod.shape), seed + 8) if c.gate else None
    return c


def resid_case_fwd(ar, c, factor=None, flips=True):
    return residual_fwd(ar, c.x_in, c.branch, c.L, w_b=c.w_b, nt=c.nt, gate=chunk(c.mod, GATE_IDX, c.d, c.B), modality=c.modality, p_drop=c.p, seed=SEED,
                        w_n=c.w_n, n_shift=chunk(c.mod_n, 0, c.d, c.B), n_scale=chunk(c.mod_n, 1, c.d, c.B), n_modality=c.n_modality, n_any_img=c.n_any_img,
                        factor=factor, flips=flips, **_win(c))


def resid_case_bwd(ar, c, fwd, factor=None, prefill=True):
    rs = fwd["rstd_b"].to(F32) if c.sandwich else None
    mu = fwd["mean_b"].to(F32) if c.sandwich and c.nt else None
    return residual_bwd(ar, c.dx, c.branch, c.L, w_b=c.w_b, rstd_b=rs, mean_b=mu, nt=c.nt, gate=chunk(c.mod, GATE_IDX, c.d, c.B), modality=c.modality,
                        dw_b0=c.dw_b0 if prefill else None, dgate0=chunk(c.dmod0, GATE_IDX, c.d, c.B) if prefill else None, p_drop=c.p, seed=SEED, factor=factor,
                        **_win(c))


def qk_heads(d):
    """head dims of the qk-norm tests at width d: D in {32, 64, 128, 256} wherever d % D == 0"""
    return [D for D in (32, 64, 128, 256) if d % D == 0 and d % 16 == 0]


def rope_tables(B, L, D, per_sample):
    pos = torch.arange(B * L if per_sample else L, dtype=F64)
    if per_sample:
        pos = (pos * 7 + 3) % 1013            # a table per sample: no two rows alike
    ang = pos[:, None] * (10000.0 ** (-torch.arange(D // 2, dtype=F64) / (D // 2)))[None]
    cos, sin = torch.cos(ang).to(F32), torch.sin(ang).to(F32)
    return (cos.view(B, L, D // 2), sin.view(B, L, D // 2)) if per_sample else (cos, sin)


def qk_case(family, B, L, d, D, qk_norm=True, per_sample=False, q_scale=1.0, seed=3):
    M = B * L
    c = types.SimpleNamespace(M=M, B=B, L=L, d=d, D=D, family=family, qk_norm=qk_norm, per_sample=per_sample, q_scale=q_scale)
    c.qkv, c.dqkr = make_rows(family, M, 3 * d, seed).to(BF16), _rn((M, 2 * d), seed + 1).to(BF16)
    c.cos, c.sin = rope_tables(B, L, D, per_sample)
    c.aff = {k: ((1 if k[0] == "g" else 0) + 0.1 * _rn((d,), seed + 2 + i)) for i, k in enumerate(("gq", "bq", "gk", "bk"))} if qk_norm else {}
    c.acc0 = {k: _rn((d,), seed + 10 + i) for i, k in enumerate(("dgq", "dbq", "dgk", "dbk"))} if qk_norm else None
    c.exact_sums = family == "ints"
    return c


def qk_case_fwd(ar, c, factor=None, flips=True):
    return qknorm_rope_fwd(ar, c.qkv, c.cos, c.sin, c.L, c.D, q_scale=c.q_scale, factor=factor, flips=flips, exact_sums=c.exact_sums, **c.aff, **_win(c))


def qk_case_bwd(ar, c, fwd, factor=None, prefill=True):
    return qknorm_rope_bwd(ar, c.dqkr, c.qkv, c.cos, c.sin, c.L, c.D, gq=c.aff.get("gq"), gk=c.aff.get("gk"), stats=fwd["stats"].to(F32) if c.qk_norm else None,
                           acc0=c.acc0 if prefill else None, q_scale=c.q_scale, factor=factor, **_win(c))


FUSED_VARIANTS = ("plain", "sandwich_rms", "sandwich_ln", "dropout")                              # udm_norm_residual_bwd: no gate, no modulation
FUSED_ADA_VARIANTS = {                                                                           # udm_norm_residual_bwd_ada: (norm mode, residual variant)
    "mod_sandwich": ("mod_all", "sandwich_rms"), "mod_img_gate_sandwich_dropout": ("mod_img", "gate_sandwich_dropout"),
    "mod_gate_plain": ("mod_all", "gate_all"), "gate_only": ("plain", "gate_img_dropout"), "mod_ln_gate": ("mod_img", "gate_img_dropout"),
}


def fused_case(family, B, L, d, mode, variant, seed=4):
    """the operands of norm_bwd (case n) and of residual_bwd (case r) of one fused launch; one norm type for both norms (the residual variant's)"""
    r = resid_case(family, B, L, d, variant, seed)
    n = norm_case("gauss", B, L, d, r.nt, mode, seed + 20)
    return types.SimpleNamespace(n=n, r=r, M=B * L, B=B, L=L, d=d, family=family, variant=variant, mode=mode, nt=r.nt)


def fused_window(c, r0, r1):
    return types.SimpleNamespace(**dict(vars(c), n=window(c.n, r0, r1), r=window(c.r, r0, r1), M=r1 - r0))


def fused_case_bwd(ar, c, stats, factor=None, prefill=True, accumulate=True):
    """stats: rstd, mean (of the norm), rstd_b, mean_b (of the sandwich norm) - the saved fp32 statistics"""
    n, r = c.n, c.r
    kw = dict(n.kw)
    if n.mod is not None and prefill:
        kw.update(dshift0=chunk(n.dmod0, MOD_IDX[0], c.d, c.B), dscale0=chunk(n.dmod0, MOD_IDX[1], c.d, c.B))
    return norm_residual_bwd(ar, n.dy, n.x, stats["rstd"].to(F32), stats["mean"].to(F32), n.w, c.nt, c.L, r.branch, dx0=n.dx0 if accumulate else None,
                             dw0=n.dw0 if prefill else None, w_b=r.w_b, rstd_b=stats["rstd_b"].to(F32) if r.sandwich else None,
                             mean_b=stats["mean_b"].to(F32) if r.sandwich and c.nt else None, dw_b0=r.dw_b0 if prefill else None, p_drop=r.p, seed=SEED,
                             gate=chunk(r.mod, GATE_IDX, c.d, c.B), dgate0=chunk(r.dmod0, GATE_IDX, c.d, c.B) if prefill else None, modality_r=r.modality,
                             factor=factor, **kw, **_win(n))


def fused_stats(ar, c):
    """the four saved statistics from the reference forwards"""
    f, g = norm_case_fwd(ar, c.n), resid_case_fwd(ar, c.r)
    z = torch.zeros(c.M, dtype=F64)
    return dict(rstd=f["rstd"], mean=f["mean"], rstd_b=g.get("rstd_b", z), mean_b=g.get("mean_b", z))
