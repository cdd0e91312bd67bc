"""In-place fp64 audit of the row-kernel and attention calls the engine makes (tests/test_engine_rowattn_audit_host.py on the CPU doubles,
tests/test_gpu_engine_rowattn_audit.py on the GPU): the counterpart of tests/engine_gemm_audit.py for `norm_fwd`, `norm_bwd`, `residual_fwd`, `residual_bwd`,
`norm_residual_bwd` (and its adaLN form), `qknorm_rope_fwd`, `qknorm_rope_bwd`, `attention_fwd` and `attention_bwd` of the module the engine calls as `K`.

Per call (the outermost one: a wrapper that runs two others inside lists them as `inner`):
  before   every operand is copied to the CPU as the kernel reads it - adaLN chunks by pointer and row stride out of the [Bp, n d] tensor, q | k out of `qkr`
           at columns 0 and d, v out of `qkv` at column 2 d - and so is the prior content of every accumulated output (dx with accumulate, dw, dw_b, the adaLN
           gradient tensor, dgq / dbq / dgk / dbk, dbias) and of every buffer only a part of which may be written (d qkv);
  after    every output is compared with the fp64 restatements that the kernel-level tests use, with the bounds THEY derive (none is measured here):
           row kernels    tests/rowops_ref64.py with `R.REF`, per element through `R.worst` at the module's FACTOR, in row chunks of 512; the backward references
                          take the fp32 statistics the kernel was handed; column sums start from the captured prior, whose term is (n + 8) EF() |prior|
                          (`bwd_all` of tests/test_gpu_rowops_rowwise.py); the bias gradient is the column sum of the kernel's own bf16 d branch;
           attention      tests/attention_ref64.py: `attention_ref64(..., prescaled=..., sample_ids=..., causal=..., zt=...)` (sample ids decoded as mask codes by
                          `pair_ok`, zt = `keep_scaled(seed, p, B, H, L)` under attention dropout), `row_errors` against `BOUNDS`, `lse_excess` for lse2;
           untouched      the v columns of d qkv after `qknorm_rope_bwd` and its q | k columns after `attention_bwd`, the columns of the adaLN gradient outside
                          the written chunks and its rows >= B, and every read-only operand keep their bits.
Each call signature - wrapper, (M, d, L) or (B, H, L, D), norm type, variant flags, output - is one row `worst error / bound <= 1`; a NaN counts as inf.

Pairing (`Auditor.pair`, the engine's own mistakes): every backward call is resolved, by the data pointers of what the forward saved (rstd, the branch, qkv,
lse), to the forward call it belongs to, and the two must agree on what the module docstring of the tests lists: norm weight, norm type, L, adaLN tensor and
chunk indices, gate index, dropout probability and seed, sample ids, doc ranges, causal flag; every forward slot (a fused residual + next-norm call has two) has
exactly one backward partner; no two dropout draws of one step share a seed."""
import contextlib
import inspect
import types

import torch

import attention_ref64 as A
import ledger
import rowops_ref64 as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
INF = float("inf")
WRAPPERS = ("norm_fwd", "norm_bwd", "residual_fwd", "residual_bwd", "norm_residual_bwd", "norm_residual_bwd_ada", "qknorm_rope_fwd", "qknorm_rope_bwd",
            "attention_fwd", "attention_bwd")
NORM = {0: "rms", 1: "ln"}
CHUNK = 512


# ------------------------------------------------------------------------------------------------ helpers
def _cpu(t):
    return None if t is None else t.detach().to("cpu").clone()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _cols(t, rows, c0, n):
    """rows x n from column c0 of a row-major 2-D tensor, through its pointer and row stride: what a kernel handed `ptr + c0` and `stride(0)` sees"""
    return t.as_strided((rows, n), (t.stride(0), 1), t.storage_offset() + c0)


def _chunk(mod, k, d, B):
    """adaLN chunk k as `_mod_ptrs` of unidisc_amd/kernels.py forms it: B rows of d from column k d, row stride of the tensor (CPU copy)"""
    return None if mod is None or k is None else _cpu(_cols(mod, B, k * d, d))


def _ranges(M):
    return [(r, min(M, r + CHUNK)) for r in range(0, M, CHUNK)]


def _sl(t, r0, r1):
    return None if t is None else t[r0:r1]


def _heads(t, B, L, H, D):
    return t.reshape(B, L, H, D).permute(0, 2, 1, 3)


def _finite_ratio(x):
    return INF if x != x else float(x)


class Auditor:
    def __init__(self, K, test, record=True):
        self.K, self.test, self.record = K, test, record
        self.calls, self.rows, self.depth, self.cur = [], {}, 0, None
        self.faults, self.fwd, self.bwd, self.draws, self.S = [], {}, [], [], None
        self.paired = False

    # ---- records
    def _row(self, call, what, ratio):
        ratio = _finite_ratio(ratio)
        key = f"{call.sig} {what}"
        self.rows[key] = max(self.rows.get(key, 0.0), ratio)
        call.ratios[what] = max(call.ratios.get(what, 0.0), ratio)

    def _cmp(self, call, key, got, ref, E, bf16=False):
        self._row(call, key, R.worst(got, ref, E, bf16)[0])

    def _new(self, name, shape, norm, flags):
        sig = f"{name} {shape}" + (f" {norm}" if norm else "") + (" " + ",".join(flags) if flags else "")
        call = types.SimpleNamespace(name=name, shape=shape, norm=norm, flags=list(flags), sig=sig, idx=len(self.calls), launches=[], inner=[], ratios={}, info={})
        self.calls.append(call)
        return call

    def _readonly(self, call, **ops):
        """bit copies of the read-only operands; the returned check runs after the call"""
        kept = [(n, t, _cpu(t)) for n, t in ops.items() if t is not None]

        def check():
            for n, t, c in kept:
                if not _same_bits(_cpu(t), c):
                    self.faults.append(f"{self.test}: {call.sig} (call {call.idx}): the read-only operand `{n}` changed")
        return check

    def _unchanged(self, call, what, got, prior, keep):
        """the elements of `got` selected by the bool mask `keep` hold the bits of `prior`"""
        if not torch.equal(_bits(got[keep]), _bits(prior[keep])):
            self.faults.append(f"{self.test}: {call.sig} (call {call.idx}): {what} changed")

    def by(self, name):
        return [c for c in self.calls if c.name == name]

    def poison_scratch(self):
        """fill the wrappers' column-reduction workspace with NaN (before a step)"""
        if hasattr(self.K, "_scratch") and torch.cuda.is_available():
            self.K._scratch(1 << 24, torch.empty(0, device="cuda").device).fill_(float("nan"))

    # ---- pairing
    def _slot(self, kind, key, call, **fields):
        if key is not None:
            self.fwd[(kind, key)] = types.SimpleNamespace(kind=kind, call=call, fields=fields, partners=[])

    def _back(self, kind, key, call, **fields):
        self.bwd.append(types.SimpleNamespace(kind=kind, key=key, call=call, fields=fields))

    def pair(self):
        """resolve every backward call to its forward call (after the backward); the failures join the audit's when it closes"""
        self.paired = True
        err = lambda m: self.faults.append(f"{self.test}: pairing: {m}")
        for b in self.bwd:
            slot = self.fwd.get((b.kind, b.key))
            who = f"{b.call.name} (call {b.call.idx}, {b.kind} half)"
            if slot is None:
                err(f"{who}: what it was handed as saved by the forward was produced by no audited forward call")
                continue
            slot.partners.append(b)
            if set(slot.fields) != set(b.fields):           # (a field recorded on one side only would never be compared)
                err(f"{who} against {slot.call.name} (call {slot.call.idx}): the two sides record different fields: {sorted(set(slot.fields) ^ set(b.fields))}")
            for f, want in slot.fields.items():
                got = b.fields.get(f)
                if f == "seed" and not (slot.fields.get("p_drop") or b.fields.get("p_drop")):
                    continue
                if got != want:
                    err(f"{who} against {slot.call.name} (call {slot.call.idx}): `{f}` differs: forward {want}, backward {got}")
        for slot in self.fwd.values():
            if len(slot.partners) != 1:
                err(f"{slot.call.name} (call {slot.call.idx}, {slot.kind} half) has {len(slot.partners)} backward partners, not one: "
                    f"{[p.call.idx for p in slot.partners]}")
        # the chain through the attention: its q | k operand is a qknorm_rope_fwd output, and qknorm_rope_bwd reads the gradient buffers attention_bwd wrote
        qkr_made = {c.info["qkr"] for c in self.by("qknorm_rope_fwd")}
        grads_made = {(c.info["dqkr"], c.info["dqkv"]) for c in self.by("attention_bwd")}
        for c in self.by("attention_fwd"):
            if c.info["qkr"] not in qkr_made:
                err(f"attention_fwd (call {c.idx}) reads a `qkr` that no audited qknorm_rope_fwd call produced")
        for c in self.by("qknorm_rope_bwd"):
            if (c.info["dqkr"], c.info["dqkv"]) not in grads_made:
                err(f"qknorm_rope_bwd (call {c.idx}) reads `dqkr` / writes `dqkv` buffers that no audited attention_bwd call wrote")
        seen = {}
        for call, seed in self.draws:
            if seed in seen:
                err(f"{call.name} (call {call.idx}) draws its dropout mask from the seed of {seen[seed].name} (call {seen[seed].idx})")
            seen[seed] = call

    def close(self):
        bad = list(self.faults)
        if self.bwd and not self.paired:
            bad.append(f"{self.test}: pairing: backward calls were audited but `pair()` was never called")
        for key, ratio in self.rows.items():
            if self.record:
                ledger.record(self.test, key + ": worst error / bound", ratio, 1.0)
            if not ratio <= 1.0:
                bad.append(f"{self.test}: {key}: worst error / bound = {ratio:.3e} exceeds 1")
        assert not bad, f"{len(bad)} failure(s) of the audited row-kernel and attention calls:\n" + "\n".join(bad)

    # ---- shared pieces
    def _mod_kw(self, mod, idx, d, B, modality, any_img):
        """reference keywords of a modulated norm, as kernels.norm_fwd / norm_bwd hand them on (modality and any_img only beside an adaLN tensor)"""
        if mod is None:
            return dict(shift=None, scale=None, modality=None, any_img=None)
        return dict(shift=_chunk(mod, idx[0], d, B), scale=_chunk(mod, idx[1], d, B), modality=_cpu(modality), any_img=_cpu(any_img))

    @staticmethod
    def _win(kw, r0, r1, M, keys=("modality",)):
        out = dict(kw, row0=r0, M_total=M)
        for k in keys:
            out[k] = _sl(kw.get(k), r0, r1)
        return out

    def _colsums(self, call, sums, priors, got, terms):
        for k, g in got.items():
            a0 = priors[k].to(F64)
            self._cmp(call, k, g, sums[k] + a0, sums["E_" + k] + (terms[k] + 8) * R.EF() * a0.abs())

    def _dmod_watch(self, call, dmod, idx, d, B):
        """prior of the adaLN gradient tensor; the returned check: columns outside the chunks `idx` and rows >= B keep their bits (`other_columns_unchanged`)"""
        if dmod is None:
            return None, lambda: None
        prior = _cpu(dmod)

        def check():
            keep = torch.ones(prior.shape, dtype=torch.bool)
            for k in idx:
                keep[:B, k * d:(k + 1) * d] = False
            self._unchanged(call, "an adaLN gradient column outside the written chunks, or a padding row,", _cpu(dmod), prior, keep)
        return prior, check

    # ---- norm
    def _a_norm_fwd(self, p):
        M, d = p.x.shape
        B, nt = -(-M // p.L), p.norm_type
        img = p.mod is not None and p.modality is not None
        call = self._new("norm_fwd", (M, d, p.L), NORM[nt], [f"mod{tuple(p.mod_idx)}" + ("/img" if img else "")] if p.mod is not None else [])
        x, w = _cpu(p.x), _cpu(p.w)
        kw = self._mod_kw(p.mod, p.mod_idx, d, B, p.modality, p.any_img)
        ro = self._readonly(call, x=p.x, w=p.w, mod=p.mod, modality=p.modality if p.mod is not None else None)

        def post(res):
            y, rstd, mean = (_cpu(t) for t in res)
            self._slot("norm", _ptr(res[1]), call, x=_ptr(p.x), w=_ptr(p.w), nt=nt, L=p.L, mod=_ptr(p.mod), mod_idx=tuple(p.mod_idx) if p.mod is not None else None,
                       modality=_ptr(p.modality) if p.mod is not None else None, mean=_ptr(res[2]))
            for r0, r1 in _ranges(M):
                ref = R.norm_fwd(R.REF, x[r0:r1], w, nt, p.L, **self._win(kw, r0, r1, M))
                self._cmp(call, "y", y[r0:r1], ref["y"], ref["E_y"], True)
                self._cmp(call, "rstd", rstd[r0:r1], ref["rstd"], ref["E_rstd"])
                if nt:
                    self._cmp(call, "mean", mean[r0:r1], ref["mean"], ref["E_mean"])
            ro()
        return call, post

    def _norm_half(self, p, call, mod, dmod, mod_idx, modality, any_img, also=()):
        """captures of a norm backward (on its own or as the first half of a fused pass) -> (reference keywords, column-sum bookkeeping, checks)"""
        M, d = p.x.shape
        B = -(-M // p.L)
        kw = self._mod_kw(mod, mod_idx, d, B, modality, any_img)
        ops = dict(dy=_cpu(p.dy), x=_cpu(p.x), rstd=_cpu(p.rstd), mean=_cpu(p.mean), w=_cpu(p.w), dx0=_cpu(p.dx) if p.accumulate else None)
        priors, terms, got = dict(dw=_cpu(p.dw)), dict(dw=M), dict(dw=lambda: _cpu(p.dw))
        dmod0, watch = self._dmod_watch(call, dmod if mod is not None else None, tuple(mod_idx) + tuple(also), d, B)
        if mod is not None:
            for k, i in zip(("dshift", "dscale"), mod_idx):
                priors[k], terms[k] = dmod0[:B, i * d:(i + 1) * d], p.L
                got[k] = lambda i=i: _chunk(dmod, i, d, B)
        self._back("norm", _ptr(p.rstd), call, x=_ptr(p.x), w=_ptr(p.w), nt=p.norm_type, L=p.L, mod=_ptr(mod), mod_idx=tuple(mod_idx) if mod is not None else None,
                   modality=_ptr(modality) if mod is not None else None, mean=_ptr(p.mean))
        return kw, ops, priors, terms, got, watch

    def _a_norm_bwd(self, p):
        M, d = p.x.shape
        nt = p.norm_type
        img = p.mod is not None and p.modality is not None
        call = self._new("norm_bwd", (M, d, p.L), NORM[nt], [f"acc{int(p.accumulate)}"] + ([f"mod{tuple(p.mod_idx)}" + ("/img" if img else "")] if p.mod is not None else []))
        kw, o, priors, terms, got, watch = self._norm_half(p, call, p.mod, p.dmod, p.mod_idx, p.modality, p.any_img)
        ro = self._readonly(call, dy=p.dy, x=p.x, rstd=p.rstd, mean=p.mean, w=p.w, mod=p.mod)

        def post(res):
            dx, sums = _cpu(p.dx), {}
            for r0, r1 in _ranges(M):
                ref = R.norm_bwd(R.REF, o["dy"][r0:r1], o["x"][r0:r1], o["rstd"][r0:r1], _sl(o["mean"], r0, r1), o["w"], nt, p.L, dx0=_sl(o["dx0"], r0, r1),
                                 **self._win(kw, r0, r1, M))
                self._cmp(call, "dx", dx[r0:r1], ref["dx"], ref["E_dx"])
                for k in priors:
                    for kk in (k, "E_" + k):
                        sums[kk] = sums.get(kk, 0) + ref[kk]
            self._colsums(call, sums, priors, {k: g() for k, g in got.items()}, terms)
            watch(), ro()
        return call, post

    # ---- residual branch
    @staticmethod
    def _gate(mod, gate_idx):
        return gate_idx if (gate_idx is not None and mod is not None) else None

    def _a_residual_fwd(self, p):
        M, d = p.x_in.shape
        B, nt, gi = -(-M // p.L), p.norm_type, self._gate(p.mod, p.gate_idx)
        flags = (["w_b"] if p.w_b is not None else []) + ([f"gate{gi}" + ("/img" if p.modality is not None else "")] if gi is not None else [])
        flags += [f"drop{p.p_drop:g}"] if p.p_drop > 0 else []
        if p.next_w is not None:
            nimg = p.next_mod is not None and p.next_modality is not None
            flags += ["next" + (f"_mod{tuple(p.next_mod_idx)}" + ("/img" if nimg else "") if p.next_mod is not None else "")]
        call = self._new("residual_fwd", (M, d, p.L), NORM[nt], flags)
        x_in, br, w_b, w_n = _cpu(p.x_in), _cpu(p.branch), _cpu(p.w_b), _cpu(p.next_w)
        gate, modality = _chunk(p.mod, gi, d, B), _cpu(p.modality)
        nkw = self._mod_kw(p.next_mod if p.next_w is not None else None, p.next_mod_idx, d, B, p.next_modality, p.next_any_img)
        ro = self._readonly(call, x_in=p.x_in, branch=p.branch, w_b=p.w_b, mod=p.mod, modality=p.modality, next_w=p.next_w, next_mod=p.next_mod)
        if p.p_drop > 0:
            self.draws.append((call, int(p.seed)))

        def post(res):
            got = dict(x_out=_cpu(res[0]), rstd_b=_cpu(res[1]), mean_b=_cpu(res[2]))
            keys = ["x_out"] + (["rstd_b"] if p.w_b is not None else []) + (["mean_b"] if p.w_b is not None and nt else [])
            # (nt: the type of the sandwich norm - without one the kernel never reads it)
            self._slot("resid", _ptr(p.branch), call, x=None, w_b=_ptr(p.w_b), nt=nt if p.w_b is not None else None, L=p.L, gate_idx=gi,
                       mod=_ptr(p.mod) if gi is not None else None, modality=_ptr(p.modality), p_drop=float(p.p_drop), seed=int(p.seed), rstd_b=_ptr(res[1]), mean_b=_ptr(res[2]))
            if p.next_w is not None:
                h, rstd_n, mean_n = res[3]
                got.update(h=_cpu(h), rstd_n=_cpu(rstd_n), mean_n=_cpu(mean_n))
                keys += ["h", "rstd_n"] + (["mean_n"] if nt else [])
                self._slot("norm", _ptr(rstd_n), call, x=_ptr(res[0]), w=_ptr(p.next_w), nt=nt, L=p.L, mod=_ptr(p.next_mod),
                           mod_idx=tuple(p.next_mod_idx) if p.next_mod is not None else None,
                           modality=_ptr(p.next_modality) if p.next_mod is not None else None, mean=_ptr(mean_n))
            for r0, r1 in _ranges(M):
                ref = R.residual_fwd(R.REF, x_in[r0:r1], br[r0:r1], p.L, w_b=w_b, nt=nt, gate=gate, modality=_sl(modality, r0, r1), p_drop=float(p.p_drop),
                                     seed=int(p.seed), w_n=w_n, n_shift=nkw["shift"], n_scale=nkw["scale"], n_modality=_sl(nkw["modality"], r0, r1),
                                     n_any_img=nkw["any_img"], row0=r0, M_total=M)
                for k in keys:
                    self._cmp(call, k, got[k][r0:r1], ref[k], ref["E_" + k], k in R.BF16_OUT)
                    if k + "_nr" in ref:
                        self._cmp(call, k + "/nr", got[k][r0:r1], ref[k + "_nr"], ref["E_" + k + "_nr"], k in R.BF16_OUT)
            ro()
        return call, post

    def _resid_half(self, p, call, branch, w_b, rstd_b, mean_b, nt, L, mod, dmod, gate_idx, modality, dw_b, p_drop, seed, M, d, also=()):
        B, gi = -(-M // L), self._gate(mod, gate_idx)
        kw = dict(w_b=_cpu(w_b), nt=nt, gate=_chunk(mod, gi, d, B), modality=_cpu(modality), p_drop=float(p_drop), seed=int(seed))
        ops = dict(branch=_cpu(branch), rstd_b=_cpu(rstd_b), mean_b=_cpu(mean_b))
        priors, terms, got = {}, {}, {}
        if w_b is not None:
            priors["dw_b"], terms["dw_b"], got["dw_b"] = _cpu(dw_b), M, lambda: _cpu(dw_b)
        dmod0, watch = self._dmod_watch(call, dmod if gi is not None else None, (gi,) + tuple(also), d, B)
        if gi is not None:
            priors["dgate"], terms["dgate"], got["dgate"] = dmod0[:B, gi * d:(gi + 1) * d], L, lambda: _chunk(dmod, gi, d, B)
        self._back("resid", _ptr(branch), call, x=None, w_b=_ptr(w_b), nt=nt if w_b is not None else None, L=L, gate_idx=gi, mod=_ptr(mod) if gi is not None else None, modality=_ptr(modality),
                   p_drop=float(p_drop), seed=int(seed), rstd_b=_ptr(rstd_b), mean_b=_ptr(mean_b))
        return kw, ops, priors, terms, got, watch

    def _a_residual_bwd(self, p):
        M, d = p.dx.shape
        nt, gi = p.norm_type, self._gate(p.mod, p.gate_idx)
        flags = (["w_b"] if p.w_b is not None else []) + ([f"gate{gi}" + ("/img" if p.modality is not None else "")] if gi is not None else [])
        call = self._new("residual_bwd", (M, d, p.L), NORM[nt] if p.w_b is not None else None, flags + ([f"drop{p.p_drop:g}"] if p.p_drop > 0 else []))
        kw, o, priors, terms, got, watch = self._resid_half(p, call, p.branch, p.w_b, p.rstd, p.mean, nt, p.L, p.mod, p.dmod, p.gate_idx, p.modality, p.dw_b,
                                                            p.p_drop, p.seed, M, d)
        dxg = _cpu(p.dx)
        ro = self._readonly(call, dx=p.dx, branch=p.branch, w_b=p.w_b, rstd=p.rstd, mean=p.mean, mod=p.mod if gi is not None else None, modality=p.modality)

        def post(res):
            db, sums = _cpu(res), {}
            for r0, r1 in _ranges(M):
                ref = R.residual_bwd(R.REF, dxg[r0:r1], o["branch"][r0:r1], p.L, rstd_b=_sl(o["rstd_b"], r0, r1), mean_b=_sl(o["mean_b"], r0, r1),
                                     **self._win(kw, r0, r1, M))
                self._cmp(call, "dbranch", db[r0:r1], ref["dbranch"], ref["E_dbranch"], True)
                for k in priors:
                    for kk in (k, "E_" + k):
                        sums[kk] = sums.get(kk, 0) + ref[kk]
            self._colsums(call, sums, priors, {k: g() for k, g in got.items()}, terms)
            watch(), ro()
        return call, post

    def _a_fused(self, p, name):
        """norm_residual_bwd and norm_residual_bwd_ada: the norm backward, then the residual-branch backward on the dx it has just updated"""
        M, d = p.x.shape
        nt, ada = p.norm_type, name.endswith("_ada")
        mod_n, dmod_n, mod_idx = (p.mod_n, p.dmod_n, p.mod_idx) if ada else (None, None, (0, 1))
        mod_r, dmod_r, gate_idx, modality_r = (p.mod_r, p.dmod_r, p.gate_idx, p.modality_r) if ada else (None, None, None, None)
        gi = self._gate(mod_r, gate_idx)
        flags = [f"acc{int(p.accumulate)}"] + (["w_b"] if p.w_b is not None else []) + ([f"drop{p.p_drop:g}"] if p.p_drop > 0 else [])
        flags += (["dbias"] if p.dbias is not None else []) + ([f"mod{tuple(mod_idx)}"] if mod_n is not None else []) + ([f"gate{gi}"] if gi is not None else [])
        call = self._new(name, (M, d, p.L), NORM[nt], flags)
        one = mod_n is not None and gi is not None and _ptr(dmod_n) == _ptr(dmod_r)       # one adaLN gradient tensor takes the chunks of both halves
        nkw, no, priors, terms, got, watch_n = self._norm_half(p, call, mod_n, dmod_n, mod_idx, p.modality if ada else None, p.any_img if ada else None,
                                                               also=(gi,) if one else ())
        rkw, ro_, pr, tr, gr, watch_r = self._resid_half(p, call, p.branch, p.w_b, p.rstd_b, p.mean_b, nt, p.L, mod_r, dmod_r, gate_idx, modality_r, p.dw_b,
                                                         p.p_drop, p.seed, M, d, also=tuple(mod_idx) if one else ())
        priors.update(pr), terms.update(tr), got.update(gr)
        dbias0 = _cpu(p.dbias)
        ro = self._readonly(call, dy=p.dy, x=p.x, rstd=p.rstd, mean=p.mean, w=p.w, branch=p.branch, w_b=p.w_b, rstd_b=p.rstd_b, mean_b=p.mean_b, mod_n=mod_n,
                            mod_r=mod_r if gi is not None else None)
        rkw = dict(rkw, modality_r=rkw.pop("modality"))
        rkw.pop("nt")

        def post(res):
            dx, db, sums = _cpu(p.dx), _cpu(res), {}
            for r0, r1 in _ranges(M):
                kw = dict(self._win(nkw, r0, r1, M), **rkw)
                kw["modality_r"] = _sl(rkw["modality_r"], r0, r1)
                ref = R.norm_residual_bwd(R.REF, no["dy"][r0:r1], no["x"][r0:r1], no["rstd"][r0:r1], _sl(no["mean"], r0, r1), no["w"], nt, p.L, ro_["branch"][r0:r1],
                                          dx0=_sl(no["dx0"], r0, r1), rstd_b=_sl(ro_["rstd_b"], r0, r1), mean_b=_sl(ro_["mean_b"], r0, r1), **kw)
                self._cmp(call, "dx", dx[r0:r1], ref["dx"], ref["E_dx"])
                self._cmp(call, "dbranch", db[r0:r1], ref["dbranch"], ref["E_dbranch"], True)
                for k in priors:
                    for kk in (k, "E_" + k):
                        sums[kk] = sums.get(kk, 0) + ref[kk]
            self._colsums(call, sums, priors, {k: g() for k, g in got.items()}, terms)
            # the bias gradient: column sums of the bf16 d branch the kernel itself wrote, in any order.  The bound is the one stated in the module docstring
            # of tests/rowops_ref64.py ("the bias gradient of the fused backward ...: (M + 8) e sum|d branch|", |acc0| counting as a term), in the form
            # `run_fused` of tests/test_gpu_rowops_rowwise.py asserts it
            if dbias0 is not None:
                d64 = db.to(F64)
                self._cmp(call, "dbias", _cpu(p.dbias), dbias0.to(F64) + d64.sum(0), (M + 8) * R.EF() * (dbias0.to(F64).abs() + d64.abs().sum(0)))
            watch_n(), watch_r(), ro()
        return call, post

    # ---- qk-norm + rotary
    def _a_qk_fwd(self, p):
        M, d = p.qkv.shape[0], p.qkv.shape[1] // 3
        qn = p.gq is not None
        call = self._new("qknorm_rope_fwd", (M, d, p.L), f"D{p.D}", [f"qk_norm{int(qn)}", f"q_scale{p.q_scale:.4g}", "rope/sample" if p.cos.dim() == 3 else "rope/L"])
        qkv, cos, sin = _cpu(p.qkv), _cpu(p.cos), _cpu(p.sin)
        aff = {k: _cpu(getattr(p, k)) for k in ("gq", "bq", "gk", "bk")}
        ro = self._readonly(call, qkv=p.qkv, cos=p.cos, sin=p.sin, gq=p.gq, bq=p.bq, gk=p.gk, bk=p.bk)

        def post(res):
            qkr, stats = _cpu(res[0]), _cpu(res[1])
            self._slot("qk", _ptr(p.qkv), call, L=p.L, D=p.D, gq=_ptr(p.gq), gk=_ptr(p.gk), cos=_ptr(p.cos), sin=_ptr(p.sin), q_scale=float(p.q_scale), stats=_ptr(res[1]))
            call.info.update(qkr=_ptr(res[0]))
            for r0, r1 in _ranges(M):
                ref = R.qknorm_rope_fwd(R.REF, qkv[r0:r1], cos, sin, p.L, p.D, q_scale=p.q_scale, row0=r0, M_total=M, **aff)
                self._cmp(call, "qkr", qkr[r0:r1], ref["qkr"], ref["E_qkr"], True)
                if qn:
                    self._cmp(call, "qkr/nr", qkr[r0:r1], ref["qkr_nr"], ref["E_qkr_nr"], True)
                    self._cmp(call, "stats", stats[r0:r1], ref["stats"], ref["E_stats"])
            ro()
        return call, post

    def _a_qk_bwd(self, p):
        M, d = p.qkv.shape[0], p.qkv.shape[1] // 3
        qn = p.gq is not None
        names = ("dgq", "dbq", "dgk", "dbk")
        one = qn and all(_ptr(getattr(p, names[i])) == _ptr(p.dgq) + 4 * d * i for i in range(4))
        call = self._new("qknorm_rope_bwd", (M, d, p.L), f"D{p.D}", [f"qk_norm{int(qn)}", f"q_scale{p.q_scale:.4g}"] + (["one_allocation" if one else "four_tensors"] if qn else []))
        dqkr, qkv, cos, sin, stats, gq, gk = (_cpu(t) for t in (p.dqkr, p.qkv, p.cos, p.sin, p.stats, p.gq, p.gk))
        dqkv0 = _cpu(p.dqkv)
        priors = {k: _cpu(getattr(p, k)) for k in names} if qn else {}
        ro = self._readonly(call, dqkr=p.dqkr, qkv=p.qkv, cos=p.cos, sin=p.sin, stats=p.stats, gq=p.gq, gk=p.gk)
        self._back("qk", _ptr(p.qkv), call, L=p.L, D=p.D, gq=_ptr(p.gq), gk=_ptr(p.gk), cos=_ptr(p.cos), sin=_ptr(p.sin), q_scale=float(p.q_scale), stats=_ptr(p.stats))
        call.info.update(dqkr=_ptr(p.dqkr), dqkv=_ptr(p.dqkv))

        def post(res):
            dqkv, sums = _cpu(p.dqkv), {}
            keep = torch.zeros(dqkv.shape, dtype=torch.bool)
            keep[:, 2 * d:] = True
            self._unchanged(call, "a v column of d qkv", dqkv, dqkv0, keep)
            for r0, r1 in _ranges(M):
                ref = R.qknorm_rope_bwd(R.REF, dqkr[r0:r1], qkv[r0:r1], cos, sin, p.L, p.D, gq=gq, gk=gk, stats=_sl(stats, r0, r1), q_scale=p.q_scale, row0=r0, M_total=M)
                self._cmp(call, "dqk", dqkv[r0:r1, :2 * d], ref["dqk"], ref["E_dqk"], True)
                for k in priors:
                    for kk in (k, "E_" + k):
                        sums[kk] = sums.get(kk, 0) + ref[kk]
            self._colsums(call, sums, priors, {k: _cpu(getattr(p, k)) for k in priors}, {k: M for k in priors})
            ro()
        return call, post

    # ---- attention
    def _attn_operands(self, p):
        """q | k from `qkr` at columns 0 and d (row stride 2 d), v from `qkv` at column 2 d (row stride 3 d): the pointers of kernels.attention_fwd"""
        B, L, H, D = p.B, p.L, p.H, p.D
        d, M = H * D, B * L
        q, k, v = (_heads(_cpu(_cols(t, M, c, d)), B, L, H, D) for t, c in ((p.qkr, 0), (p.qkr, d), (p.qkv, 2 * d)))
        sid = _cpu(p.sample_ids)
        zt = A.keep_scaled(int(p.seed) & 0xFFFFFFFFFFFFFFFF, float(p.dropout_p), B, H, L) if p.dropout_p else None
        flags = [f"prescaled{int(bool(p.q_prescaled))}", f"causal{int(bool(p.causal))}"] + (["codes" + ("+ranges" if p.doc_ranges is not None else "")] if sid is not None else [])
        flags += [f"attn_drop{p.dropout_p:g}"] if p.dropout_p else []
        fields = dict(qkr=_ptr(p.qkr), qkv=_ptr(p.qkv), shape=(B, L, H, D), sample_ids=_ptr(p.sample_ids), doc_ranges=_ptr(p.doc_ranges), q_prescaled=bool(p.q_prescaled),
                      causal=bool(p.causal), dropout_p=float(p.dropout_p), seed=int(p.seed), p_drop=float(p.dropout_p))
        return q, k, v, sid, zt, flags, fields

    def _a_attn_fwd(self, p):
        B, L, H, D = p.B, p.L, p.H, p.D
        q, k, v, sid, zt, flags, fields = self._attn_operands(p)
        call = self._new("attention_fwd", (B, H, L, D), None, flags)
        call.info.update(sample_ids=_ptr(p.sample_ids), doc_ranges=_ptr(p.doc_ranges), qkr=_ptr(p.qkr))
        ro = self._readonly(call, qkr=p.qkr, qkv=p.qkv, sample_ids=p.sample_ids, doc_ranges=p.doc_ranges)
        if p.dropout_p:
            self.draws.append((call, int(p.seed)))

        def post(res):
            o, lse = res
            self._slot("attn", _ptr(lse), call, o=_ptr(o), **fields)
            ref = A.attention_ref64(q, k, v, None, prescaled=bool(p.q_prescaled), sample_ids=sid, causal=bool(p.causal), zt=zt)
            self._row(call, "o", A.row_errors(_heads(_cpu(o), B, L, H, D), ref["o"], ref["sc_o"])[0] / A.BOUNDS["o"])
            excess, _, dead_ok = A.lse_excess(_cpu(lse).reshape(B, H, L), ref)
            self._row(call, "lse2", excess if dead_ok else INF)
            ro()
        return call, post

    def _a_attn_bwd(self, p):
        B, L, H, D = p.B, p.L, p.H, p.D
        d, M = H * D, B * L
        q, k, v, sid, zt, flags, fields = self._attn_operands(p)
        call = self._new("attention_bwd", (B, H, L, D), None, flags)
        call.info.update(sample_ids=_ptr(p.sample_ids), doc_ranges=_ptr(p.doc_ranges), dqkr=_ptr(p.dqkr), dqkv=_ptr(p.dqkv))
        do = _heads(_cpu(_cols(p.do, M, 0, d)), B, L, H, D)
        dqkv0 = _cpu(p.dqkv)
        ro = self._readonly(call, qkr=p.qkr, qkv=p.qkv, o=p.o, do=p.do, lse=p.lse, sample_ids=p.sample_ids, doc_ranges=p.doc_ranges)
        self._back("attn", _ptr(p.lse), call, o=_ptr(p.o), **fields)

        def post(res):
            ref = A.attention_ref64(q, k, v, do, prescaled=bool(p.q_prescaled), sample_ids=sid, causal=bool(p.causal), zt=zt)
            dqkv = _cpu(p.dqkv)
            got = dict(dq=_cpu(_cols(p.dqkr, M, 0, d)), dk=_cpu(_cols(p.dqkr, M, d, d)), dv=dqkv[:, 2 * d:])
            for key, g in got.items():
                self._row(call, key, A.row_errors(_heads(g, B, L, H, D), ref[key], ref["sc_" + key])[0] / A.BOUNDS[key])
            keep = torch.zeros(dqkv.shape, dtype=torch.bool)
            keep[:, :2 * d] = True
            self._unchanged(call, "a q | k column of d qkv", dqkv, dqkv0, keep)
            ro()
        return call, post

    # ---- the wrapper
    def wrap(self, name, orig):
        from unidisc_amd import kernels as real

        sig = inspect.signature(getattr(real, name))                 # (the doubles and their mutants take the arguments of the wrapper they stand in for)
        pre = {"norm_fwd": self._a_norm_fwd, "norm_bwd": self._a_norm_bwd, "residual_fwd": self._a_residual_fwd, "residual_bwd": self._a_residual_bwd,
               "norm_residual_bwd": lambda p: self._a_fused(p, "norm_residual_bwd"), "norm_residual_bwd_ada": lambda p: self._a_fused(p, "norm_residual_bwd_ada"),
               "qknorm_rope_fwd": self._a_qk_fwd, "qknorm_rope_bwd": self._a_qk_bwd, "attention_fwd": self._a_attn_fwd, "attention_bwd": self._a_attn_bwd}[name]

        def audited(*args, **kw):
            if self.depth:
                self.cur.inner.append(name)
                return orig(*args, **kw)
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            call, post = pre(types.SimpleNamespace(**ba.arguments))
            self.depth, self.cur = 1, call
            try:
                res = orig(*args, **kw)
            finally:
                self.depth, self.cur = 0, None
            post(res)
            return res

        return audited


def _missing(name):
    def missing(*a, **k):
        raise AssertionError(f"the engine reached K.{name}, which the kernel doubles do not provide: the audited step cannot run on them")
    return missing


@contextlib.contextmanager
def audit(monkeypatch, K, test, record=True):
    """Audit every row-kernel and attention call made through module `K` (unidisc_amd.kernels or tests/fake_kernels.py) inside the block.  `aud.S` is the `_Saved`
    of the last forward (its sid, doc_ranges, p_drop, p_attn).  Call `aud.pair()` after the backward; the rows and the pairing are asserted - and, with `record`,
    the rows written to the ledger - when the block ends."""
    from unidisc_amd.dit import DIT

    aud = Auditor(K, test, record)
    with monkeypatch.context() as mp:
        for name in WRAPPERS:
            if hasattr(K, name):
                mp.setattr(K, name, aud.wrap(name, getattr(K, name)))
            else:
                mp.setattr(K, name, _missing(name), raising=False)
        lib = getattr(K, "_lib", None)
        if lib is not None:
            lib_call = lib.call

            def spy(entry, *a, **k):
                if aud.cur is not None:
                    aud.cur.launches.append(entry)
                return lib_call(entry, *a, **k)

            mp.setattr(lib, "call", spy)
        masks = DIT._attention_masks

        def masks_seen(self, S, inp, dev):
            aud.S = S
            return masks(self, S, inp, dev)

        mp.setattr(DIT, "_attention_masks", masks_seen)
        yield aud
    aud.close()


def entries(aud):
    """the library entry points the audited calls launched"""
    return {e for c in aud.calls for e in c.launches}


def worst_by_family(aud):
    """worst ratio per kernel family (the RESULTS.md table)"""
    fam = dict(norm=0.0, residual=0.0, fused=0.0, qknorm_rope=0.0, attention=0.0)
    for c in aud.calls:
        k = "fused" if c.name.startswith("norm_residual") else c.name.split("_")[0] if not c.name.startswith("qknorm") else "qknorm_rope"
        fam[k] = max([fam[k]] + list(c.ratios.values()))
    return fam


# ------------------------------------------------------------------------------------------------ the models of the two test files
def build(model, device, case=None, **attrs):
    """`build` of tests/engine_gemm_audit.py (seeded weights, head and adaLN weights randomised) on `cases()[model]` updated by `case`, then every norm weight
    (and qk-norm bias) moved off its initial 1 (0): with the initial values a norm handed another norm's weight computes the same thing.  `attrs`: attributes of
    the backbone set after construction (dropout, attn_dropout)."""
    import engine_gemm_audit as E

    diff = E.build(model, device, case=case)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if "norm" in n and p.dim() == 1:
                p.add_((0.1 * torch.randn(p.shape, generator=g)).to(device))
    for k, v in attrs.items():
        assert hasattr(diff.backbone, k), k
        setattr(diff.backbone, k, v)
    return diff
