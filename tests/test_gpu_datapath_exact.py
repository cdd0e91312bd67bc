"""The batch-preparation and loss kernels on a real MI355X (pytest -m gpu), straight through `unidisc_amd._lib.call` on caller-owned buffers: joint assembly,
timestep / noise schedule, the absorbing mask, the packed-row rope and block lottery (csrc/tokens.hip), the attention document ranges (csrc/attention.hip) and
the diffusion loss (csrc/ce.hip) - every output element against the serial / fp64 statements of tests/datapath_ref.py, out of guarded buffers.

Memory discipline.  Every operand, output and scratch buffer has its exact stated size and sits between guard regions: floats in the NaN arenas of gemm_ref64,
integers and bools between 256 sentinel bytes (0xA5) each side, outputs and scratch prefilled with the same poison.  After each call: the guards are intact, the
inputs bit-identical, every element the contract says is written no longer holds the poison, every element it leaves alone still does.  What is written:
  rope scratch [B, 5, L] int32      planes 0 (run start), 1 (run end), 3 (id-run start) everywhere; plane 2 (j) at image-run starts; plane 4 the first n_starts entries
  lottery scratch [B, 4, L] int32   planes 0 (block start), 1 (block end) everywhere; plane 2 the first n_candidates entries; plane 3 at candidate starts
  row_cands [B] int32 everywhere;   n_cand by the last row's workgroup (one store);  row flags of udm_qxt_absorbing only when a draw is given
Every kernel is launched twice on the same buffers and must repeat itself bit for bit - udm_diffusion_loss included: one workgroup, a fixed summation order, no
atomics.  Exact: everything integer or bool, t, dsigma, nlls, the counts.  Bounded (datapath_ref derives the bounds): sigma, the move chance, the loss scalars and
coef; the ledger gets achieved / bound.  The tests of these kernels against the product's fallback path stay where they are (test_gpu_kernels.py,
test_gpu_interleaved_kernels.py): that is another statement.
"""
import ctypes

import numpy as np
import pytest
import torch

import datapath_ref as D
import gemm_ref64 as G
import ledger

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "datapath_exact"
F32 = torch.float32
F32N, F64N = np.float32, np.float64
GUARD_ROWS, GUARD_BYTES, POISON = 16, 256, 0xA5
LAYOUTS = D.layout_cases()


def call(name, *args):
    from unidisc_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class Mem:
    """the buffers of one call"""

    def __init__(self):
        self.arenas, self.raws, self.inputs, self.outputs = [], [], [], []

    def _f(self, shape):
        n = int(np.prod(shape))
        s2 = (n // shape[-1], shape[-1]) if len(shape) > 1 else (1, n)
        a = G.arena(s2, s2[1], F32, guard_rows=GUARD_ROWS, device=DEV)
        assert a.view.data_ptr() % 16 == 0 and a.view.is_contiguous()
        self.arenas.append(a)
        return a.view.view(shape)

    def _i(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw = torch.full((2 * GUARD_BYTES + n,), POISON, dtype=torch.uint8, device=DEV)
        self.raws.append((raw, n))
        return raw[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape)

    def inp(self, a):
        """a numpy operand (fp32, or any integer / bool - bools travel as bytes) at its exact size"""
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8) if a.dtype == bool else a))
        v = self._f(tuple(t.shape)) if t.dtype == F32 else self._i(tuple(t.shape), t.dtype)
        v.copy_(t)
        self.inputs.append((v, t))
        return v

    def out(self, shape, dtype=F32):
        v = self._f(tuple(shape)) if dtype == F32 else self._i(tuple(shape), dtype)
        self.outputs.append(v)
        return v

    def check(self, what):
        """(strays, changed inputs) - both asserted 0"""
        torch.cuda.synchronize()
        strays = sum(G.stray_count(a) for a in self.arenas)
        strays += sum(int((r[:GUARD_BYTES] != POISON).sum()) + int((r[GUARD_BYTES + n:] != POISON).sum()) for r, n in self.raws)
        changed = sum(int(v.cpu().contiguous().numpy().tobytes() != t.contiguous().numpy().tobytes()) for v, t in self.inputs)
        assert strays == 0, f"{what}: {strays} guard elements changed"
        assert changed == 0, f"{what}: {changed} input operands changed"
        return strays + changed

    def snapshot(self):
        torch.cuda.synchronize()
        return [v.cpu().contiguous().numpy().tobytes() for v in self.outputs]


def written(t):
    """bool numpy array: the elements that no longer hold the poison"""
    c = t.detach().cpu().contiguous()
    if c.dtype == F32:
        return (c.view(torch.int32) != G.NAN_BITS[F32]).numpy()
    return (c.view(torch.uint8).reshape(*c.shape, c.element_size()) != POISON).any(-1).numpy()


def np_(t):
    return t.detach().cpu().numpy()


class Tally:
    """the figures of one test: asserted case by case, recorded once (integers against 0, ratios against 1)"""

    def __init__(self, key):
        self.key, self.n = key, {}

    def count(self, name, n, what):
        self.n[name] = self.n.get(name, 0) + int(n)
        assert n == 0, f"{self.key} {what}: {name} = {n}"

    def ratio(self, name, q, what):
        self.n[name] = max(self.n.get(name, 0.0), float(q))
        assert q <= 1.0, f"{self.key} {what}: {name} = {q:.3f} of its bound"

    def write_set(self, name, t, expect, what):
        """`expect`: True (all), or a bool array - exactly these elements are written"""
        w = written(t)
        e = np.ones(w.shape, bool) if expect is True else expect
        self.count(f"{name} unwritten", int((e & ~w).sum()), what)
        self.count(f"{name} written outside the contract", int((~e & w).sum()), what)

    def close(self, cases):
        ledger.check(TEST, f"{self.key} cases", 0, 0, note=f"{cases} calls, each launched twice")
        for name, v in self.n.items():
            ledger.check(TEST, f"{self.key} {name}", v, 1.0 if isinstance(v, float) else 0)


def twice(mem, t, launch, what):
    """launch, snapshot, check; launch again on the same buffers: bit-identical"""
    launch()
    first = mem.snapshot()
    t.count("strays / changed inputs", mem.check(what), what)
    launch()
    t.count("second launch differs", sum(int(a != b) for a, b in zip(first, mem.snapshot())), what)
    t.count("strays / changed inputs", mem.check(what + " (second launch)"), what)


# ------------------------------------------------------------------------------------------------ joint assembly
def test_assemble_joint_tokens():
    t = Tally("assemble_joint_tokens")
    cases = D.assemble_cases()
    for c in cases:
        what = c["name"]
        Lt, Li, B = c["txt"].shape[1], c["img"].shape[1], c["B"]
        mem = Mem()
        txt, tm, img, idx = mem.inp(c["txt"]), mem.inp(c["txt_mask"]), mem.inp(c["img"]), mem.inp(c["idx"])
        ids, mask, mod = mem.out((B, Lt + Li), torch.int64), mem.out((B, Lt + Li), torch.uint8), mem.out((B, Lt + Li), torch.int64)
        twice(mem, t, lambda: call("udm_assemble_joint_tokens", ptr(txt), ptr(tm), ptr(img), ptr(idx), B, Lt, Li, c["Vt"], ptr(ids), ptr(mask), ptr(mod)), what)
        ref = D.assemble_ref(c["txt"], c["txt_mask"], c["img"], c["idx"], B, c["Vt"])
        for name, got, r in zip(("ids", "mask", "modality"), (ids, mask, mod), ref):
            t.write_set(name, got, True, what)
            t.count("mismatches", D.same(np_(got), r.astype(np_(got).dtype)), f"{what} {name}")
    t.close(len(cases))


# ------------------------------------------------------------------------------------------------ absorbing mask
@pytest.mark.parametrize("B,L", D.QXT_SHAPES)
def test_qxt_absorbing(B, L):
    t = Tally(f"qxt_absorbing B={B} L={L}")
    cases = [c for c in D.qxt_cases() if c["x"].shape == (B, L)]
    assert [c["name"].split("-")[-1] for c in cases] == list(D.QXT_DRAWS)
    for c in cases:
        what = c["name"]
        drawn = c["r_txt"] is not None or c["r_img"] is not None
        mem = Mem()
        x, rm, mc, rt, ri = mem.inp(c["x"]), mem.inp(c["r_move"]), mem.inp(c["mc"]), mem.inp(c["r_txt"]), mem.inp(c["r_img"])
        mm = mem.inp(c["mm"]) if drawn else None
        xt, move = mem.out((B, L), torch.int64), mem.out((B, L), torch.uint8)
        rows = [mem.out((B,), torch.uint8) for _ in range(3)] if drawn else [None] * 3
        twice(mem, t, lambda: call("udm_qxt_absorbing", ptr(x), ptr(rm), ptr(mc), ptr(rt), ptr(ri), float(c["thr_txt"]), float(c["thr_img"]), ptr(mm), B, L, c["mask_id"],
                                   ptr(xt), ptr(move), ptr(rows[0]), ptr(rows[1]), ptr(rows[2])), what)
        ref = D.qxt_ref(c["x"], c["r_move"], c["mc"], c["r_txt"], c["r_img"], c["thr_txt"], c["thr_img"], c["mm"], c["mask_id"])
        for name, got, r in zip(("xt", "move", "row_txt", "row_img", "row_ignore"), (xt, move, *rows), ref):
            if got is not None:
                t.write_set(name, got, True, what)
                t.count("mismatches", D.same(np_(got), r.astype(np_(got).dtype)), f"{what} {name}")
    t.close(len(cases))


# ------------------------------------------------------------------------------------------------ document ranges
def test_attention_doc_ranges():
    t = Tally("attention_doc_ranges")
    cases = D.doc_cases()
    for c in cases:
        what = c["name"]
        B, L = c["sid"].shape
        mem = Mem()
        sid, out = mem.inp(c["sid"]), mem.out((B, (L + 63) // 64, 8), torch.int32)
        twice(mem, t, lambda: call("udm_attention_doc_ranges", ptr(sid), B, L, ptr(out)), what)
        t.write_set("ranges", out, True, what)
        t.count("mismatches", D.same(np_(out), D.doc_ranges_ref(c["sid"])), what)
    t.close(len(cases))


# ------------------------------------------------------------------------------------------------ timestep and noise schedule
@pytest.mark.parametrize("n", D.T_NOISE_N)
def test_sample_t_noise(n):
    t = Tally(f"sample_t_noise n={n}")
    c, eps, c1 = (float(v) for v in D.t_noise_consts())
    calls = 0
    for antithetic in (False, True):
        for seed in (0, 1):
            what = f"antithetic={antithetic} seed={seed}"
            u_np = D.t_noise_u(n, seed)
            mem = Mem()
            u = mem.inp(u_np)
            outs = [mem.out((n,)) for _ in range(4)]
            twice(mem, t, lambda: call("udm_sample_t_noise", ptr(u), n, int(antithetic), c, eps, c1, *[ptr(o) for o in outs]), what)
            calls += 1
            for name, o in zip(("t", "sigma", "dsigma", "move"), outs):
                t.write_set(name, o, True, what)
            tt, sg, ds, mv = (np_(o) for o in outs)
            t_ref, ds_ref = D.t_noise_ieee(u_np, antithetic)
            t.count("t mismatches", D.same(tt, t_ref), what)
            t.count("dsigma mismatches", D.same(ds, ds_ref), what)
            s64, m64, Es, Em = D.t_noise_64(tt)                       # at the kernel's own t (equal to the statement's, asserted above)
            t.ratio("sigma err/bound", D.ratio(sg, s64, D.FACTOR * D.W_SIGMA * Es), what)
            t.ratio("move err/bound", D.ratio(mv, m64, D.FACTOR * D.W_MOVE * Em), what)
            for k, v in D.t_noise_properties(tt, mv, antithetic).items():
                t.count(f"property {k}", v, what)
    t.close(calls)


# ------------------------------------------------------------------------------------------------ packed rows: rope
@pytest.mark.parametrize("L", D.LENGTHS)
def test_interleaved_rope(L):
    t = Tally(f"interleaved_rope L={L}")
    calls = 0
    for c in (c for c in LAYOUTS if c["L"] == L):
        B = c["mod"].shape[0]
        for nsizes, half in D.ROPE_CONFIGS:
            what = f"{c['name']} nsizes={nsizes} half={half} rows={c['rows']}"
            sizes, ic, isn, tc, ts = D.rope_tables(nsizes, half)
            mem = Mem()
            mod, sid = mem.inp(c["mod"]), mem.inp(c["sid"])
            tabs = [mem.inp(a) for a in (ic, isn, tc, ts)]
            cos, sin, cidx = mem.out((B, L, half)), mem.out((B, L, half)), mem.out((B, L), torch.int64)
            scratch = mem.out((B, 5, L), torch.int32)
            hs = (ctypes.c_int32 * max(len(sizes), 1))(*sizes)            # a host array
            twice(mem, t, lambda: call("udm_interleaved_rope", ptr(mod), ptr(sid), ptr(tabs[0]), ptr(tabs[1]), hs, len(sizes), ptr(tabs[2]), ptr(tabs[3]), D.TXT_ROWS, B, L,
                                       half, ptr(cos), ptr(sin), ptr(cidx), ptr(scratch)), what)
            calls += 1
            src, row, j, starts = D.rope_ref(c["mod"], c["sid"], sizes, D.TXT_ROWS)
            for name, got, r in (("cos", cos, D.rope_apply(src, row, ic, tc)), ("sin", sin, D.rope_apply(src, row, isn, ts)), ("count_idx", cidx, j)):
                t.write_set(name, got, True, what)
                t.count("mismatches", D.same(np_(got), r), f"{what} {name}")
            expect = np.zeros((B, 5, L), bool)
            expect[:, [0, 1, 3]] = True
            for b in range(B):
                expect[b, 2, starts[b]] = True
                expect[b, 4, :len(starts[b])] = True
            t.write_set("scratch", scratch, expect, what)
    t.close(calls)


# ------------------------------------------------------------------------------------------------ packed rows: block lottery
@pytest.mark.parametrize("L", D.LENGTHS)
def test_interleaved_block_lottery(L):
    t = Tally(f"interleaved_block_lottery L={L}")
    calls = 0
    for c in (c for c in LAYOUTS if c["L"] == L):
        B = c["mod"].shape[0]
        n_cand = D.lottery_ref(c["mod"], c["sid"], None, 0, 0.5)[2]
        for k, (p, n_r) in enumerate(D.lottery_configs(n_cand)):
            what = f"{c['name']} p={p} n_r={n_r} of {n_cand} rows={c['rows']}"
            r_np = D.lottery_uniforms(c["mod"], c["sid"], p, n_r, seed=L + k)
            mem = Mem()
            mod, sid, r = mem.inp(c["mod"]), mem.inp(c["sid"]), (mem.inp(r_np) if n_r else None)
            accum, rows_hit, nc = mem.out((B, L), torch.uint8), mem.out((B,), torch.uint8), mem.out((1,), torch.int64)
            scratch, row_cands = mem.out((B, 4, L), torch.int32), mem.out((B,), torch.int32)
            twice(mem, t, lambda: call("udm_interleaved_block_lottery", ptr(mod), ptr(sid), ptr(r), n_r, float(F32N(p)), B, L, ptr(accum), ptr(rows_hit), ptr(nc),
                                       ptr(scratch), ptr(row_cands)), what)
            calls += 1
            acc_ref, rows_ref, n_ref, _, cstarts = D.lottery_ref(c["mod"], c["sid"], r_np, n_r, p)
            assert n_ref == n_cand
            for name, got, ref in (("accum", accum, acc_ref.astype(np.uint8)), ("rows_hit", rows_hit, rows_ref.astype(np.uint8)), ("n_cand", nc, np.array([n_ref])),
                                   ("row_cands", row_cands, np.array([len(s) for s in cstarts], np.int32))):
                t.write_set(name, got, True, what)
                t.count("mismatches", D.same(np_(got), ref), f"{what} {name}")
            expect = np.zeros((B, 4, L), bool)
            expect[:, [0, 1]] = True
            for b in range(B):
                expect[b, 2, :len(cstarts[b])] = True
                expect[b, 3, cstarts[b]] = True
            t.write_set("scratch", scratch, expect, what)
    t.close(calls)


# ------------------------------------------------------------------------------------------------ diffusion loss
def _loss_call(c, B, L, log_p):
    mem = Mem()
    kw = c["kw"]
    lp, wl, ws, att, mm = mem.inp(log_p), mem.inp(c["w_loss"]), mem.inp(c["w_std"]), mem.inp(c["att"]), mem.inp(c["mm"])
    nlls, coef, sc = mem.out((B, L)), mem.out((B, L)), mem.out((8,))
    ratio = -1.0 if kw.get("ratio") is None else float(kw["ratio"])
    launch = lambda: call("udm_diffusion_loss", ptr(lp), ptr(wl), ptr(ws), ptr(att), ptr(mm), ptr(nlls), ptr(coef), ptr(sc), B, L, int(kw["weighted"]),
                          int(kw.get("full_mask", False)), float(kw["text_w"]), float(kw["img_w"]), ratio)
    return mem, launch, (nlls, coef, sc)


@pytest.mark.parametrize("B,L", D.LOSS_SHAPES)
def test_diffusion_loss(B, L):
    """Figures of the first run on an MI355X (worst achieved / bound over the cases of a shape) are in profiles/datapath_exact_parity_ledger.json."""
    t = Tally(f"diffusion_loss {B}x{L}")
    for case in D.LOSS_CASES:
        what = case
        c = D.loss_case(B, L, case)
        ref = D.loss_ref(c["log_p"], c["w_loss"], c["w_std"], c["att"], c["mm"], **c["kw"])
        mem, launch, outs = _loss_call(c, B, L, c["log_p"])
        twice(mem, t, launch, what)                                    # one workgroup, fixed order, no atomics: the second launch repeats the first bit for bit
        for name, o in zip(("nlls", "coef", "scalars"), outs):
            t.write_set(name, o, True, what)
        nlls, coef, sc = (np_(o) for o in outs)
        bad, q = D.loss_judge(B * L, case, nlls, coef, sc, ref)
        print(f"diffusion_loss {B}x{L} {case}: mismatches {bad}, achieved / bound {q}")
        t.count("nlls / count mismatches", bad, what)
        for k, v in q.items():
            t.ratio(f"{k} err/bound", v, what)
        behind = ~c["att"]
        if not c["kw"].get("full_mask"):
            # behind the mask: nlls is +0, coef is -w x 0 = -0 (w > 0 here); NaN there changes nothing, bit for bit
            t.count("coef behind the mask is not -0", int((~np.signbit(coef[behind]) | (coef[behind] != 0)).sum()), what)
            t.count("nlls behind the mask is not +0", int((np.signbit(nlls[behind]) | (nlls[behind] != 0)).sum()), what)
            if behind.any():
                mem2, launch2, outs2 = _loss_call(c, B, L, np.where(c["att"], c["log_p"], F32N("nan")))
                launch2()
                t.count("strays / changed inputs", mem2.check(what + " (NaN behind the mask)"), what)
                t.count("NaN behind the mask changes an output", sum(int(not torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))) for a, b in zip(outs, outs2)),
                        what)
    t.close(len(D.LOSS_CASES))
