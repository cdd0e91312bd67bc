"""In-place fp64 audit of the GEMM-class calls the engine makes (tests/test_engine_gemm_audit_host.py on the CPU doubles, tests/test_gpu_engine_gemm_audit.py on
the GPU): `audit(...)` wraps the GEMM wrappers of the module the engine calls as `K`, rebuilds every call's logical operands from its arguments as the kernel sees
them (M, N, K, leading dimensions, epilogue, beta, bias, aux), runs the real wrapper, and compares the result on the CPU with the fp64 product.

No bound here is measured on the code under test.  With S = |A| |B| (the fp64 product of the absolute values), n the contraction length and u = 2^-24:

  fp32 output      |got - ref| <= a,  a = (n + 8) u S: bf16 x bf16 products are exact in fp32, only the accumulation rounds (the form of attention_ref64.py's
                   lse2); the + 8 absorbs the split-K slice sums and the reduce pass.  beta = 1: the prior |C| joins S and its term n; EPI_BIAS: so does the bias.
  bf16 output      a + half_ulp(|ref| + a): round-to-nearest of an fp32 accumulator within a.  half_ulp(x) = 2^(e - 8) for 2^e <= x < 2^(e + 1) is half the spacing
                   of bf16's 8-bit significand, between 2^-9 x and 2^-8 x.  (A flat 2^-9 |ref| is NOT a bound of a correct rounding: it holds only in the upper
                   end of a binade; the exact fp32 emulations of tests/test_engine_gemm_audit_host.py miss it by up to 1.94 x.)
  exact operands   integer-valued A, B (bias, prior) with S < 2^24: every fp32 partial sum is exact, a = 0, and a bf16 output must BE the round-to-nearest-even of
                   the reference (this is what tells a kernel that rounds ties away from zero from one that rounds them to even).
  EPI_BIAS_GELU    csrc/gemm.hip stores in `aux` NOT the pre-activation but bf16(gelu'(u)), u = bf16(acc + bias), and writes C = bf16(gelu(u)) (gelu_tanh_both of
                   csrc/common.h); EPI_DGELU then is a single multiply by the stored derivative.  u itself is never stored, so the audit brackets it: rounding is
                   monotone, u lies between lo = bf16(ref - a) and hi = bf16(ref + a).  Where hi is lo or its bf16 successor (all but elements within a few
                   2^-8 a of zero) u is one of the two and (C, aux) must match gelu64 / dgelu64 of ONE of them within `gelu_bound` of tests/gemm_ref64.py - the
                   bound of the kernel-level tests - plus, for aux, the gelu' formula term below; elsewhere 1.13 (hi - lo) is added (1.13 = max |gelu'|, and
                   max |gelu''| = 0.80 is below it).
  gelu' formula    the fp32 evaluation of gelu' in gelu_tanh_both against dgelu64, transcribed to torch fp32 and swept over every bf16 value in [-12, 12]
                   (`dgelu_formula_term`): worst |formula - dgelu64| = 1.48e-07 (at u = 1.15625); 2 x that = 2.95e-07 is the term (two fp32 evaluation orders differ
                   by less).  It applies where the formula runs: to the `aux` output of EPI_BIAS_GELU.
  EPI_DGELU        C = round(acc * aux) with aux as stored: reference acc64 * aux, S scaled by |aux|, one more term for the product's rounding.  The `bias`
                   argument receives the column sums of the values AS STORED (csrc/gemm.hip sums the bf16-rounded words it is about to store; the fp32 values for
                   an fp32 output): reference = prior + the fp64 column sums of the audited output, with the fp32 summation bound over M + 1 terms.
  small_batch_linear_bwd   csrc/rowops.hip rounds the fp32 `dmod` to bf16 on load, before every product and before the bias column sums; the reference does the
                   same.  dW = d16^T X (n = B), db = prior + colsum(d16) (n = B + 1), sum of dx_parts = d16 W (n = out): the fp32 rule each.

Comparisons are by value and a NaN fails (ratio = inf).  Every call signature adds one `ledger.check` row (worst error / bound <= 1) when the audit closes."""
import contextlib
import functools
import inspect
import types

import torch

import gemm_ref64 as R
import ledger

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU = 0, 1, 2, 3
EPI_NAME = {EPI_NONE: "none", EPI_BIAS: "bias", EPI_BIAS_GELU: "bias_gelu", EPI_DGELU: "dgelu"}
GELU_LIP = 1.13                # max |gelu'| (tanh form), attained near u = 1.5
WRAPPERS = ("gemm_nt", "gemm_nn", "gemm_tn", "gemm_tn_splitk", "gemm_nt_splitk", "gemm_nn_splitk", "gemm_tn_pair", "gemm_tn_multi", "small_batch_linear_bwd")
INF = float("inf")


# ------------------------------------------------------------------------------------------------ bounds
def acc_bound(S, n):
    """fp32 summation of n exact terms whose absolute values sum to S"""
    return (n + 8) * U * S


def half_ulp_bf16(x):
    """half the spacing of bf16 at |x| (fp64): 2^(e - 8) for 2^e <= |x| < 2^(e + 1); 0 at 0"""
    m, e = torch.frexp(x.abs())                                      # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 9))


def bf16_bound(ref, a):
    return half_ulp_bf16(ref.abs() + a) + a


def worst_ratio(err, bound):
    """largest err / bound; 0 / 0 counts as 0, anything over a zero bound and every NaN as inf"""
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, INF), r)
    return float(r.max())


def dgelu_formula_f32(x):
    """gelu'(x) as gelu_tanh_both (csrc/common.h) evaluates it, statement by statement in torch fp32"""
    f = lambda v: torch.tensor(v, dtype=F32)
    x = x.to(F32)
    k0, k1 = f(0.7978845608028654), f(0.044715)
    c0 = f(-2.0) * f(1.4426950408889634) * k0
    c1 = c0 * k1
    x2 = x * x
    e = torch.exp2(torch.minimum(x * (c0 + c1 * x2), f(80.0)))
    s = f(1.0) / (f(1.0) + e)
    g = x * s
    return s + (g * (e * s)) * (f(2.0) * k0 + f(6.0) * k0 * k1 * x2)


@functools.lru_cache(maxsize=1)
def dgelu_formula_term():
    """2 x the worst |fp32 formula - dgelu64| over every bf16 value in [-12, 12]"""
    u = R.all_bf16_between(-12.0, 12.0)
    return 2.0 * float((dgelu_formula_f32(u).to(F64) - R.dgelu64(u)).abs().max())


def _integers(*ts):
    return all(t is None or bool((t == t.round()).all()) for t in ts)


def product_ref(A, B, *, bias=None, prior=None, beta=0.0):
    """(ref, S, n, exact) of A [M, K] B [N, K]^T (+ bias) (+ beta prior), all fp64"""
    ref, S, n = A @ B.t(), A.abs() @ B.abs().t(), A.shape[1]
    if bias is not None:
        ref, S, n = ref + bias[None, :], S + bias.abs()[None, :], n + 1
    if beta != 0.0:
        ref, S, n = ref + beta * prior, S + (beta * prior).abs(), n + 1
    exact = _integers(A, B, bias, prior if beta != 0.0 else None) and abs(beta) in (0.0, 1.0) and (S.numel() == 0 or float(S.max()) < R.LIMIT)
    return ref, S, n, exact


def check_product(got, A, B, *, bias=None, prior=None, beta=0.0):
    """worst error / bound of `got` (fp32 or bf16, CPU) against the fp64 product; the exact rule where it applies"""
    ref, S, n, exact = product_ref(A, B, bias=bias, prior=prior, beta=beta)
    a = torch.zeros_like(S) if exact else acc_bound(S, n)
    err = (got.to(F64) - ref).abs()
    if got.dtype != BF16:                                            # fp32, or an fp64 sum of fp32 partial tiles: the fp32 rule
        return worst_ratio(err, a)
    if exact and R.mismatches(got, R.rne_bf16(ref))[0]:
        return INF
    return worst_ratio(err, bf16_bound(ref, a))


def _bf16_succ(x):
    """the next bf16 value towards +inf (x bf16, finite)"""
    x = (x.float() + 0.0).to(BF16)                                   # -0 -> +0
    bits = x.view(torch.int16).to(torch.int32)
    return torch.where(x.float() >= 0, bits + 1, bits - 1).to(torch.int16).view(BF16)


def check_gelu(got_c, got_aux, A, B, bias):
    """EPI_BIAS_GELU: (ratio of C, ratio of aux) with the pre-activation bracketed as the module docstring says"""
    ref, S, n, _ = product_ref(A, B, bias=bias)
    a = acc_bound(S, n) + 2.0 ** -22 * ref.abs()                     # (+ 2^-22 |ref|: torch casts fp64 -> bf16 through fp32; the margin keeps the bracket outside)
    lo, hi = (ref - a).to(BF16), (ref + a).to(BF16)
    near = hi.float() <= _bf16_succ(lo).float()
    gap = torch.where(near, torch.zeros_like(ref), GELU_LIP * (1.0 + 2.0 ** -8) * (hi.to(F64) - lo.to(F64)))
    term = (1.0 + 2.0 ** -8) * dgelu_formula_term()
    ec = ea = None
    for c in (lo.to(F64), hi.to(F64)):
        yc, ya = R.gelu64(c), R.dgelu64(c)
        rc = (got_c.to(F64) - yc).abs() / (R.gelu_bound(yc) + gap)
        ra = (got_aux.to(F64) - ya).abs() / (R.gelu_bound(ya) + term + gap)
        rc, ra = (torch.where(torch.isnan(r), torch.full_like(r, INF), r) for r in (rc, ra))
        if ec is None:
            ec, ea = rc, ra
        else:                                                        # the candidate that fits BOTH outputs best
            better = torch.maximum(rc, ra) < torch.maximum(ec, ea)
            ec, ea = torch.where(better, rc, ec), torch.where(better, ra, ea)
    return float(ec.max()), float(ea.max())


def check_dgelu(got_c, A, B, aux, colsum_prior=None, colsum_got=None):
    """EPI_DGELU: (ratio of C, ratio of the column sums or None)"""
    ref, S, n, _ = product_ref(A, B)
    ref, S, n = ref * aux, S * aux.abs(), n + 1
    a = acc_bound(S, n)
    err = (got_c.to(F64) - ref).abs()
    rc = worst_ratio(err, a if got_c.dtype == F32 else bf16_bound(ref, a))
    if colsum_got is None:
        return rc, None
    stored = got_c.to(F64)
    cs_ref, cs_S = colsum_prior + stored.sum(0), colsum_prior.abs() + stored.abs().sum(0)
    return rc, worst_ratio((colsum_got.to(F64) - cs_ref).abs(), acc_bound(cs_S, stored.shape[0] + 1))


# ------------------------------------------------------------------------------------------------ the auditor
def _cpu(t):
    return t.detach().to("cpu").clone()


def _c64(t):
    return t.detach().to("cpu").to(F64)


def _view(t, rows, cols, ld):
    """rows x cols with row stride ld from the tensor's first element: what the kernel reads or writes through the pointer"""
    return t.as_strided((rows, cols), (ld, 1), t.storage_offset())


def _span(t, rows=None, cols=None, ld=None):
    if t is None:
        return None
    if rows is None:
        n = t.numel() if t.is_contiguous() else (t.shape[0] - 1) * t.stride(0) + t.shape[-1]
    else:
        n = (rows - 1) * ld + cols if rows else 0
    return (t.data_ptr(), t.data_ptr() + n * t.element_size())


class Auditor:
    def __init__(self, K, test, record=True, keep_io=False):
        self.K, self.test, self.record, self.keep_io = K, test, record, keep_io
        self.calls, self.rows, self.depth, self.cur = [], {}, 0, None
        self.flat, self.ranges, self.numels = None, None, None
        self.operands = {}                                           # after resolve(): parameter name -> [(dY [K, M] bf16, X [K, N] bf16)] of its weight-gradient calls

    # ---- records
    def _row(self, call, what, ratio):
        key = f"{call.name} {call.shape} epi={EPI_NAME[call.epi]} beta={call.beta:g} {what}"
        self.rows[key] = max(self.rows.get(key, 0.0), ratio)
        call.ratios[what] = max(call.ratios.get(what, 0.0), ratio)

    def _new(self, name, shape, outs, *, epi=EPI_NONE, beta=0.0, b=None):
        call = types.SimpleNamespace(name=name, shape=shape, epi=epi, beta=float(beta), outs=[o for o in outs if o is not None], b_ptr=b.data_ptr() if b is not None else None,
                                     launches=[], inner=[], ratios={}, grads=[], weight=None, result=None, wgrad=[], c0=None, io=None)
        self.calls.append(call)
        return call

    def resolve(self, bb):
        """after the backward: which parameter gradient every output belongs to, which weight shadow every `b` operand is; returns the calls"""
        spans = [(n, p.grad.data_ptr(), p.grad.data_ptr() + p.grad.numel() * 4) for n, p in bb.named_parameters() if p.grad is not None]
        shadows = []
        for ln, lin in bb._lins.items():
            for kind in ("w16", "w16t"):
                t = getattr(lin, kind, None)
                if t is not None:
                    shadows.append((ln, kind, t, *_span(t)))
        for c in self.calls:
            if not c.grads:
                c.grads = [n for n, lo, hi in spans for o in c.outs if o[0] < hi and lo < o[1]]
            if c.weight is None and c.b_ptr is not None:
                for ln, kind, t, lo, hi in shadows:
                    if lo <= c.b_ptr < hi:
                        c.weight = (ln, kind)
                        c.c0 = (c.b_ptr - lo) // (t.stride(0) * t.element_size()) if kind == "w16" else (c.b_ptr - lo) // t.element_size() % t.stride(0)
            for (lo_hi, dy, x) in c.wgrad:
                for n, lo, hi in spans:
                    if lo_hi[0] < hi and lo < lo_hi[1]:
                        self.operands.setdefault(n, []).append((dy, x))
            c.wgrad = []
        return self.calls

    def by(self, name=None, grad=None, weight=None):
        return [c for c in self.calls if (name is None or c.name == name) and (grad is None or grad in c.grads) and (weight is None or c.weight == weight)]

    def padding_gaps(self):
        """the alignment gaps behind every parameter's gradient in the flat buffer of the last backward"""
        return [self.flat[lo + self.numels[k]:hi] for k, (lo, hi) in self.ranges.items()]

    def poison_scratch(self):
        """fill the library's split-K workspace with NaN (before a step)"""
        if hasattr(self.K, "_scratch") and torch.cuda.is_available():
            self.K._scratch(1 << 24, torch.empty(0, device="cuda").device).fill_(float("nan"))

    def close(self):
        bad = []
        for key, ratio in self.rows.items():
            if self.record:
                ledger.record(self.test, key + ": worst error / bound", ratio, 1.0)
            if not ratio <= 1.0:
                bad.append(f"{self.test}: {key}: worst error / bound = {ratio:.3e} exceeds 1")
        assert not bad, f"{len(bad)} audited GEMM call signature(s) outside their fp64 bound:\n" + "\n".join(bad)

    # ---- per-wrapper audits: each returns post(result)
    def _product(self, call, what, got, A, B, **kw):
        self._row(call, what, check_product(got, A, B, **kw))

    def _nt(self, a, b, out, M, N, Kd, lda, ldb, ldc, epi, bias, aux, ldaux, beta):
        A, B = _c64(_view(a, M, Kd, lda)), _c64(_view(b, N, Kd, ldb))
        bias_in = _c64(bias[:N]) if epi in (EPI_BIAS, EPI_BIAS_GELU) else None
        cs_prior = _c64(bias[:N]) if (epi == EPI_DGELU and bias is not None) else None
        aux_in = _c64(_view(aux, M, N, ldaux)) if epi == EPI_DGELU else None
        prior = _c64(_view(out, M, N, ldc)) if (beta != 0.0 and out is not None) else None

        def post(res, call):
            ld = res.stride(0) if ldc is None else ldc
            call.outs.append(_span(res, M, N, ld))
            got = _cpu(_view(res, M, N, ld))
            if self.keep_io:                                         # bit-exact (a [M, K], b [N, K], out) for the tests that compare two runs
                call.io = (_cpu(_view(a, M, Kd, lda)), _cpu(_view(b, N, Kd, ldb)), got)
            if epi == EPI_BIAS_GELU:
                call.outs.append(_span(aux, M, N, ldaux))
                rc, ra = check_gelu(got, _cpu(_view(aux, M, N, ldaux)), A, B, bias_in)
                self._row(call, "C", rc), self._row(call, "aux", ra)
            elif epi == EPI_DGELU:
                if cs_prior is not None:
                    call.outs.append(_span(bias[:N]))
                rc, rs = check_dgelu(got, A, B, aux_in, cs_prior, _cpu(bias[:N]) if cs_prior is not None else None)
                self._row(call, "C", rc)
                if rs is not None:
                    self._row(call, "column sums", rs)
            else:
                self._product(call, "C", got, A, B, bias=bias_in, prior=prior, beta=beta)
            if res.dtype == F32:                                     # a weight gradient through the transposes of `_wgrad`: operands in the K-major form of the others
                call.wgrad.append((_span(res, M, N, ld), _cpu(_view(a, M, Kd, lda)).t().contiguous(), _cpu(_view(b, N, Kd, ldb)).t().contiguous()))
        return post

    def _tn_problem(self, call, a, b, out, M, N, beta, tag=""):
        A, B = _c64(a[:, :M]).t(), _c64(b[:, :N]).t()
        o = _view(out, M, N, out.stride(0))
        prior = _c64(o) if beta != 0.0 else None
        dy, x, span = _cpu(a[:, :M]), _cpu(b[:, :N]), _span(out, M, N, out.stride(0))
        call.outs.append(span)

        def post():
            self._product(call, "C" + tag, _cpu(o), A, B, prior=prior, beta=beta)
            call.wgrad.append((span, dy, x))
        return post

    def _small_batch(self, call, dy, x, w16, dw, db, dx, dx_parts):
        out = dy.shape[1]
        D, X, W = _c64(dy).to(BF16).to(F64), _c64(x), _c64(w16[:out])   # (fp32 -> bf16 of torch: round-to-nearest-even, as rbf of the kernel)
        db0 = _c64(db) if db is not None else None
        dx0 = _c64(dx) if (dx is not None and dx_parts is None) else None
        call.outs += [_span(dw)] + ([_span(db)] if db is not None else [])

        def post():
            self._product(call, "dW", _cpu(dw), D.t().contiguous(), X.t().contiguous())
            if db is not None:
                ones = torch.ones(1, D.shape[0], dtype=F64)
                self._product(call, "db", _cpu(db)[None, :], ones, D.t().contiguous(), prior=db0[None, :], beta=1.0)
            if dx_parts is not None:
                self._product(call, "sum of dx_parts", _c64(dx_parts).sum(0), D, W.t().contiguous())
            else:
                self._product(call, "dx", _cpu(dx), D, W.t().contiguous(), prior=dx0, beta=1.0)
        return post

    # ---- the wrapper
    def wrap(self, name, orig):
        from unidisc_amd import kernels as real

        sig = inspect.signature(getattr(real, name))                 # (the doubles and their mutants take the arguments of the wrapper they stand in for)

        def audited(*args, **kw):
            if self.depth:
                self.cur.inner.append(name)
                return orig(*args, **kw)
            p = types.SimpleNamespace(**_bind(sig, args, kw))
            posts = []
            if name == "gemm_nt":
                M = p.a.shape[0] if p.M is None else p.M
                Kd = p.a.shape[1] if p.K is None else p.K
                N = p.b.shape[0] if p.N is None else p.N
                lda = p.a.stride(0) if p.lda is None else p.lda
                ldb = p.b.stride(0) if p.ldb is None else p.ldb
                ldc = p.ldc if p.ldc is not None else (p.out.stride(0) if p.out is not None else None)
                ldaux = p.ldaux if p.ldaux is not None else (p.aux.stride(0) if p.aux is not None else None)
                call = self._new(name, (M, N, Kd), [], epi=p.epilogue, beta=p.beta, b=p.b)
                post = self._nt(p.a, p.b, p.out, M, N, Kd, lda, ldb, ldc, p.epilogue, p.bias, p.aux, ldaux, p.beta)
                posts.append(lambda res: post(res, call))
            elif name == "gemm_nt_splitk":
                (M, Kd), N = p.a.shape, (p.b.shape[0] if p.N is None else p.N)
                call = self._new(name, (M, N, Kd), [], b=p.b)
                post = self._nt(p.a, p.b, p.out, M, N, Kd, p.a.stride(0), p.b.stride(0), p.out.stride(0) if p.out is not None else None, EPI_NONE, None, None, None, 0.0)
                posts.append(lambda res: post(res, call))
            elif name in ("gemm_nn", "gemm_nn_splitk"):
                (M, Kd), N = p.a.shape, (p.b.shape[1] if p.N is None else p.N)
                call = self._new(name, (M, N, Kd), [], b=p.b)
                A, B = _c64(p.a), _c64(p.b[:, :N]).t()

                def post_nn(res, call=call, A=A, B=B, M=M, N=N):
                    call.outs.append(_span(res, M, N, res.stride(0)))
                    got = _cpu(_view(res, M, N, res.stride(0)))
                    if self.keep_io:
                        call.io = (A.to(BF16), B.to(BF16), got)
                    self._product(call, "C", got, A, B)
                posts.append(post_nn)
            elif name in ("gemm_tn", "gemm_tn_splitk"):
                Kd = p.a.shape[0]
                M, N = (p.a.shape[1] if p.M is None else p.M), (p.b.shape[1] if p.N is None else p.N)
                call = self._new(name, (M, N, Kd), [], beta=p.beta)
                post = self._tn_problem(call, p.a, p.b, p.out, M, N, p.beta)
                posts.append(lambda res: post())
            elif name == "gemm_tn_pair":
                call = self._new(name, (tuple(p.out0.shape), tuple(p.out1.shape), p.a0.shape[0]), [], beta=p.beta)
                for i, (a, b, o) in enumerate(((p.a0, p.b0, p.out0), (p.a1, p.b1, p.out1))):
                    post = self._tn_problem(call, a, b, o, o.shape[0], o.shape[1], p.beta, tag=str(i))
                    posts.append(lambda res, post=post: post())
            elif name == "gemm_tn_multi":
                call = self._new(name, (tuple(tuple(o.shape) for _, _, o in p.problems), p.problems[0][0].shape[0]), [], beta=p.beta)
                pp = [self._tn_problem(call, a, b, o, o.shape[0], o.shape[1], p.beta, tag=str(i)) for i, (a, b, o) in enumerate(p.problems)]
                posts.append(lambda res, pp=pp: [q() for q in pp] if res else None)   # (False: nothing was launched, the caller issues the plain calls)
            else:
                call = self._new(name, (p.dy.shape[0], p.dy.shape[1], p.x.shape[1]), [])
                post = self._small_batch(call, p.dy, p.x, p.w16, p.dw, p.db, p.dx, p.dx_parts)
                posts.append(lambda res: post())
            self.depth, self.cur = 1, call
            try:
                res = orig(*args, **kw)
            finally:
                self.depth, self.cur = 0, None
            call.result = res if isinstance(res, bool) else None     # (never the tensor: a second owner makes autograd clone the gradient it is handed)
            for finish in posts:
                finish(res)
            return res

        return audited


def _bind(sig, args, kw):
    ba = sig.bind(*args, **kw)
    ba.apply_defaults()
    return dict(ba.arguments)


@contextlib.contextmanager
def audit(monkeypatch, K, test, poison=True, record=True, keep_io=False):
    """Audit every GEMM-class call made through module `K` (unidisc_amd.kernels or tests/fake_kernels.py) inside the block; with `poison`, `DIT._alloc_grads` hands
    out GEMM-weight gradients filled with NaN (the other ranges stay as it made them).  The rows are asserted - and, with `record`, written to the ledger -
    when the block ends."""
    from unidisc_amd.dit import DIT

    aud = Auditor(K, test, record, keep_io)
    with monkeypatch.context() as mp:
        for name in WRAPPERS:
            if hasattr(K, name):
                mp.setattr(K, name, aud.wrap(name, getattr(K, name)))
        lib = getattr(K, "_lib", None)
        if lib is not None:
            lib_call = lib.call

            def spy(entry, *a, **k):
                if aud.cur is not None:
                    aud.cur.launches.append(entry)
                return lib_call(entry, *a, **k)

            mp.setattr(lib, "call", spy)
        alloc = DIT._alloc_grads

        def alloc_poisoned(self, params, dev):
            flat, G = alloc(self, params, dev)
            if poison:
                for lin in self._lins.values():
                    G[id(lin.weight)].fill_(float("nan"))
            names = {id(p): n for n, p in self.named_parameters()}
            aud.flat, aud.ranges = flat, {names[k]: v for k, v in self._grad_ranges.items()}
            aud.numels = {names[id(p)]: p.numel() for p in params}
            return flat, G

        mp.setattr(DIT, "_alloc_grads", alloc_poisoned)
        yield aud
    aud.close()


# ------------------------------------------------------------------------------------------------ the models of the two test files
def cases():
    from test_gpu_fullwidth_oracle import _PLUMB

    mm = dict(hidden_size=256, n_heads=4, cond_dim=128, txt_length=64, img_length=64, text_vocab_size=1001, vocab_size=1001 + 512, norm_type="rms", qk_norm=True,
              sandwich_normalization=True, modality_embed=True, rope_2d=False, time_conditioning=False, multimodal_batches=True, force_argmax_valid_indices=True,
              mask_entire_modality=0.1, softmin_snr=5, text_loss_weight=1.0, img_loss_weight=None, force_full_attention_mask_loss_only=True, n_blocks=2)
    return dict(plain=dict(_PLUMB, n_blocks=2, time_conditioning=False), plain_adaln=dict(_PLUMB, n_blocks=2, time_conditioning=True), mm=mm)


def build(model, device, case=None):
    """seeded weights, head and adaLN weights randomised (the reference zero-initialises them), as `_product` of tests/test_gpu_shadow_lifecycle.py;
    `case`: config keys on top of `cases()[model]` (tests/engine_rowattn_audit.py: the modality masking probabilities)"""
    from product_utils import product_config
    from unidisc_amd import Diffusion

    torch.manual_seed(0)
    diff = Diffusion(product_config(dict(cases()[model], **(case or {}))), None, device)
    diff.backbone.train()
    diff.rng_device = "cpu"
    wg = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "adaLN_modulation" in n:
                p.copy_((torch.randn(p.shape, generator=wg) * (0.5 / p.shape[-1] ** 0.5)).to(device))
    return diff


def batch(model, B, seed=77):
    from test_gpu_fullwidth_oracle import _make_batch

    return _make_batch(cases()[model], B, torch.Generator().manual_seed(seed))


def step(diff, b, seed=123):
    """one training_step + backward; returns the detached (loss, nlls)"""
    torch.manual_seed(seed)
    out = diff.training_step({k: v.clone() for k, v in b.items()}, 1)
    out.loss.backward()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return out.loss.detach().clone(), out.nlls.detach().clone()
