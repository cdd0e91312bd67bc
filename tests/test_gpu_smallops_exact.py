"""The small kernels around the DiT blocks on a real MI355X (pytest -m gpu), through unidisc_amd.kernels: token embedding forward / backward, rowgroup_sum, the
timestep embedding, SiLU forward / backward, the two casts of the gradient wire, the bf16 transpose with its column sums, and the cast-transpose (single and
multi) - every output element against the fp64 / IEEE statements of tests/smallops_ref64.py, exactly or inside the bounds derived there, out of NaN arenas.

Memory discipline.  Every floating-point operand and every output is a view between NaN guard rows (gemm_ref64.arena), with NaN pad columns where the entry
point takes a leading dimension; overwritten outputs start as NaN, accumulated outputs from a random tensor that the reference adds to; after each call every
arena is searched for strays and every input compared bit for bit.  Arena bases are 16-byte aligned (the guard is a multiple of 16 rows).

Which shape reaches which branch
  embedding_fwd   d = 4 (one lane), 192, 260 (a second pass of one lane), 1024, 2048; M = 1, 5 (waves without a row), 8200 rows (past 2048 blocks x 4 rows);
                  V = 1; ids -1, -100, V, V + 7 read rows 0 and V - 1 - the rows before and behind the table are NaN; `out=` into an arena
  embedding_bwd   d = 1028, 2048, 4096: grid.y = 2, 2, 4 (1028: one thread of the second column chunk); M = 1, 7 (less than one 8-row group), 128, 129 (a one-row
                  block), 1000 (a ragged last block); hot share 0, 1/2, 1; a block whose hot rows cancel to 0; hot_id outside the table
  rowgroup_sum    d = 4, 72 (ragged 64-column chunk), 64, 768; G = 1, 3, 32, 16; runs of 37 rows, one across the 512-row block seam; indices -1 and G
  casts           n = 1 .. 5, 1023 .. 1025, 4099: every tail length n % 4, on both sides of a 1024-element block
  transpose       8 x 8 (one ragged tile), 72 x 136, 200 x 72 (ragged tiles in both directions), 64 x 64; leading dimensions padded by 8
  cast_transpose  65 x 64 (a one-row tile), 67 x 67 (C % 4 != 0, R % 8 != 0), 130 x 520, 8 x 192; ld_in = C, C + 1 (scalar loads), aligned + 4;
                  ld_out / ld_t multiples of 128 (vector stores), odd (scalar stores), and one of each in the same call (ld_t = 128 k + 4: % 4 == 0 but
                  not % 8, the scalar transposed store; ld_out = 128 k + 2: scalar row stores beside vector transposed ones)
Subnormals: the elements whose statement meets a subnormal (input, intermediate or result) are asserted under keys of their own (`... subnormal ...`).
"""
import pytest
import torch

import gemm_ref64 as G
import ledger
import smallops_ref64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEST = "smallops_exact"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 16
V, HOT = S.EMB_V, S.EMB_HOT


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


def _2d(t):
    return tuple(t.shape) if t.dim() == 2 else (1, t.numel())


class Mem:
    """the arenas of one call: inputs are compared bit for bit afterwards, everything is searched for strays"""

    def __init__(self):
        self.arenas, self.inputs = [], []

    def _new(self, shape, ld, dtype, fill, guard):
        a = G.arena(shape, ld or shape[1], dtype, guard_rows=guard, device=DEV, fill=None if fill is None else fill.reshape(shape))
        assert a.view.data_ptr() % 16 == 0
        self.arenas.append(a)
        return a

    def inp(self, t, ld=None):
        a = self._new(_2d(t), ld, t.dtype, t, GUARD)
        self.inputs.append((a, t.reshape(_2d(t)).clone()))
        return a.view if t.dim() == 2 else a.view[0]

    def acc(self, t, ld=None):
        a = self._new(_2d(t), ld, t.dtype, t, GUARD)
        return a.view if t.dim() == 2 else a.view[0]

    def out(self, shape, dtype, ld=None, guard=GUARD):
        s2 = tuple(shape) if len(shape) == 2 else (1, shape[0])
        a = self._new(s2, ld, dtype, None, guard)
        return a.view if len(shape) == 2 else a.view[0]

    def strays(self, what):
        torch.cuda.synchronize()
        n = sum(G.stray_count(a) for a in self.arenas)
        assert n == 0, f"{what}: {n} elements outside the views changed"
        for a, t in self.inputs:
            assert torch.equal(a.view.cpu().view(G.INT_VIEW[a.dtype]), t.view(G.INT_VIEW[a.dtype])), f"{what}: an input operand changed"
        return n


def is_poison(t):
    """bool: the elements that still hold the arena's NaN payload"""
    return t.contiguous().view(G.INT_VIEW[t.dtype]).cpu() == torch.tensor(G.NAN_BITS[t.dtype], dtype=torch.int32).to(G.INT_VIEW[t.dtype])


class Tally:
    """the figures of the cases of one test: asserted case by case (with the case in the message), recorded once"""

    def __init__(self, key):
        self.key, self.n = key, {}

    def exact(self, name, got, ref, what, mask=None):
        g, r = got.detach().cpu(), ref
        if mask is not None:
            g, r = g[mask], r[mask]
        n, where = S.mismatches(g, r)
        self.n[name] = self.n.get(name, 0) + n
        assert n == 0, f"{self.key} {what}: {name}: {n} elements differ from the statement, first at {where}: got {[float(g[tuple(w)]) for w in where]}, " \
                       f"statement {[float(r[tuple(w)]) for w in where]}"

    def count(self, name, n, what):
        self.n[name] = self.n.get(name, 0) + int(n)
        assert n == 0, f"{self.key} {what}: {name} = {n}"

    def ratio(self, name, q, what):
        self.n[name] = max(self.n.get(name, 0.0), q)
        assert q <= 1.0, f"{self.key} {what}: {name} = {q:.3f} of its bound"

    def close(self, note=None):
        for name, v in self.n.items():
            ledger.check(TEST, f"{self.key} {name}", v, 1.0 if isinstance(v, float) else 0, note)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("d,M,V_", [(d, M, 11) for d in S.EMB_FWD_D for M in (1, 5)] + [(64, 8200, 11), (192, 5, 1)])
def test_embedding_fwd(K, d, M, V_):
    t = Tally(f"embedding_fwd d={d} M={M} V={V_}")
    for with_mod in (False, True):
        what = f"modality={with_mod}"
        ids = torch.randint(0, V_, (M,), generator=torch.Generator().manual_seed(d + M))
        if M >= 5:
            ids[0], ids[1], ids[M - 2], ids[M - 1] = -1, -100, V_, V_ + 7
            ids[M // 2] = V_ - 1
        else:
            ids[0] = V_ + 7 if with_mod else -1
        mod = S.make_modality(M, d)
        E, Em = S.gauss((V_, d), d + 1), S.gauss((2, d), d + 2)
        mem = Mem()
        Ev, Emv, x = mem.inp(E), mem.inp(Em) if with_mod else None, mem.out((M, d), F32)
        ret = K.embedding_fwd(ids.to(DEV), Ev, mod.to(DEV) if with_mod else None, Emv, out=x)
        assert ret is x
        ref = S.embedding_fwd_ref(ids, E, mod if with_mod else None, Em if with_mod else None)
        t.count("strays", mem.strays(what), what)
        t.exact("mismatches", x, ref, what)
        if M <= 5:
            t.exact("mismatches", K.embedding_fwd(ids.to(DEV), Ev, mod.to(DEV) if with_mod else None, Emv), ref, what + " (own output)")
    t.close()


def _bwd_call(K, t, family, ids, mod, dx, dE0, dEm0, hot, what):
    mem = Mem()
    dxv, dE = mem.inp(dx), mem.acc(dE0)
    dEm = mem.acc(dEm0) if dEm0 is not None else None
    K.embedding_bwd(ids.to(DEV), dxv, dE, hot, mod.to(DEV) if dEm0 is not None else None, dEm)
    ref = S.embedding_bwd_ref(ids, dx, dE0, mod, dEm0)
    t.count("strays", mem.strays(what), what)
    for k, got in (("dE", dE), ("dEm", dEm)):
        if got is None:
            continue
        if family == "ints":
            t.exact(f"{k} mismatches", got, ref[k], what)
        else:
            t.ratio(f"{k} err/bound", S.sum_ratio(got, ref[k], ref["A_" + k], ref["n_" + k]), what)
    return dE, ref


@pytest.mark.parametrize("family", ("ints", "gauss"))
@pytest.mark.parametrize("d", S.EMB_BWD_D)
def test_embedding_bwd(K, family, d):
    """out-of-range ids (rows 1, 3, M - 2, M - 1 from M = 7 on) are dropped from dE and counted in dEm"""
    t = Tally(f"embedding_bwd {family} d={d}")
    for mi, M in enumerate(S.EMB_BWD_M):
        for si, share in enumerate((0.0, 0.5, 1.0)):
            ids, mod, dx, dE0, dEm0, _ = S.emb_case(family, d, M, share)
            with_dEm = (mi + si) % 2 == 0
            _bwd_call(K, t, family, ids, mod, dx, dE0, dEm0 if with_dEm else None, HOT, f"M={M} hot share={share} dEm={with_dEm}")
    t.close()


@pytest.mark.parametrize("family", ("ints", "gauss"))
@pytest.mark.parametrize("d,M", [(4, 7), (192, 129), (1028, 128), (2048, 1000)])
def test_embedding_bwd_cancelled_hot_block(K, family, d, M):
    """the hot rows of the first block cancel exactly to 0 (adjacent +-pairs, the kernel's own order) and no other block has a hot row: the table row of hot_id
    equals its starting value"""
    t = Tally(f"embedding_bwd cancelled {family} d={d} M={M}")
    ids, mod, dx, dE0, dEm0, _ = S.emb_case(family, d, M, 0.5)
    ids, dx = S.cancelling_hot_block(ids, dx, HOT, V)
    assert int((ids == HOT).sum()) >= 2
    dE, _ = _bwd_call(K, t, family, ids, mod, dx, dE0, dEm0, HOT, "cancelling block")
    t.exact("hot row mismatches", dE[HOT], dE0[HOT], "the hot row against its starting value")
    t.close()


@pytest.mark.parametrize("hot", (-1, V))
@pytest.mark.parametrize("d,M", [(4, 129), (1028, 129)])
def test_embedding_bwd_hot_id_out_of_range(K, hot, d, M):
    """a hot_id outside [0, V) means "no hot row": the ids equal to it are dropped like every out-of-range id, nothing is stored before or behind the table
    (the guard of 16 rows holds a whole table row: even a store at row -1 or V would have stayed inside the allocation)"""
    t = Tally(f"embedding_bwd hot_id={hot} d={d} M={M}")
    for family in ("ints", "gauss"):
        ids, mod, dx, dE0, dEm0, _ = S.emb_case(family, d, M, 0.0)
        ids[::3] = hot
        ids[-1] = hot
        _bwd_call(K, t, family, ids, mod, dx, dE0, dEm0, hot, family)
    t.close()


# ------------------------------------------------------------------------------------------------ rowgroup_sum
@pytest.mark.parametrize("family", ("ints", "gauss"))
@pytest.mark.parametrize("M,d,G_", S.ROWGROUP)
def test_rowgroup_sum(K, family, M, d, G_):
    t = Tally(f"rowgroup_sum {family} M={M} d={d} G={G_}")
    grp = S.make_groups(M, G_)
    if family == "ints":
        x, f = S.ints(M, d, 5)
        o0 = S.ints_like((G_, d), f, 6)
    else:
        x, o0 = S.gauss((M, d), 7), S.gauss((G_, d), 8)
    x, o0 = x.to(F32), o0.to(F32)
    mem = Mem()
    xv, out = mem.inp(x), mem.acc(o0)
    K.rowgroup_sum(xv, grp.to(DEV), out)
    ref, A, n = S.rowgroup_ref(x, grp, o0)
    t.count("strays", mem.strays(""), "")
    if family == "ints":
        t.exact("mismatches", out, ref, "")
    else:
        t.ratio("err/bound", S.sum_ratio(out, ref, A, n), "")
    t.close()


# ------------------------------------------------------------------------------------------------ timestep embedding
@pytest.mark.parametrize("dim", S.TIMESTEP_DIMS)
@pytest.mark.parametrize("B", S.TIMESTEP_B)
def test_timestep_embedding(K, B, dim):
    t = Tally(f"timestep_embedding B={B} dim={dim}")
    Bp = (B + 7) // 8 * 8
    for fam, W in (("schedule", S.W_TIMESTEP), ("far", S.W_TIMESTEP_FAR)):
        sg = S.sigmas(B, fam, dim)
        mem = Mem()
        sv, out = mem.inp(sg), mem.out((Bp, dim), BF16)
        K.timestep_embedding(sv, out, B, dim)
        ref, Sc = S.timestep_ref(sg, dim)
        E = S.timestep_E(Sc, W)
        t.count("strays", mem.strays(fam), fam)
        t.count("rows past B written", int((~is_poison(out[B:])).sum()), fam)
        got = out[:B]
        bad = S.outside(got, ref, E)
        t.count(f"outside the interval ({fam})", int(bad.sum()), f"{fam}: first at {bad.nonzero()[:4].tolist()}")
        t.ratio(f"achieved/E ({fam})", S.worst_ratio(got, ref, E), fam)
    t.close(note=f"E = {S.FACTOR} W 2^-24 (|ref| + 10 |arg| |dref/darg|), W = {S.W_TIMESTEP} (sigma <= 7), {S.W_TIMESTEP_FAR} (sigma <= 1000)")


# ------------------------------------------------------------------------------------------------ SiLU
def test_silu_fwd(K):
    """every finite bf16 bit pattern; the elements whose input or result is a subnormal under a key of their own; the `n=` prefix form"""
    t = Tally("silu_fwd all finite bf16")
    x = S.all_finite_bf16()
    n = x.numel()
    ref, Sc = S.silu_ref(x)
    E = S.silu_E(Sc)
    sub = S.subnormal_mask(x) | (ref.abs() < S.MIN_NORMAL) | (S.round_bf16_64(ref).abs() < S.MIN_NORMAL)
    for prefix in (40001, None):
        what = f"n={prefix}"
        k = n if prefix is None else prefix
        mem = Mem()
        xv, y = mem.inp(x), mem.out((n,), BF16)
        assert K.silu_fwd(xv, n=prefix, out=y) is y
        t.count("strays", mem.strays(what), what)
        t.count("elements past n written", int((~is_poison(y[k:])).sum()) if k < n else 0, what)
        bad = S.outside(y[:k], ref[:k], E[:k])
        b_norm, b_sub = bad & ~sub[:k], bad & sub[:k]
        t.count("outside the interval", int(b_norm.sum()), f"{what}: x = {x[:k][b_norm][:6].tolist()}, got {y[:k].cpu()[b_norm][:6].tolist()}, ref {ref[:k][b_norm][:6].tolist()}")
        t.count("subnormal outside the interval", int(b_sub.sum()),
                f"{what}: x = {x[:k][b_sub][:6].tolist()}, got {y[:k].cpu()[b_sub][:6].tolist()}, ref {ref[:k][b_sub][:6].tolist()}")
        a = S.achieved(y[:k], ref[:k])
        q = torch.where((a == 0) | sub[:k], torch.zeros_like(a), a / E[:k])
        t.ratio("achieved/E", float(q.max()), what)
    t.close(note=f"E = {S.FACTOR} x {S.W_SILU_FWD} x 2^-24 |ref| (1 + |x| (1 - s))")
    assert torch.equal(K.silu_fwd(x.to(DEV)).cpu().view(torch.int16), y.cpu().view(torch.int16))          # the wrapper's own output


def test_silu_bwd(K):
    t = Tally("silu_bwd all finite bf16")
    x = S.all_finite_bf16()
    for i, dy in enumerate(S.silu_dys(x.numel())):
        what = f"dy={S.SILU_DY[i]}" if i < len(S.SILU_DY) else "dy=random"
        mem = Mem()
        xv, dyv, dx = mem.inp(x), mem.inp(dy), mem.out((x.numel(),), BF16)
        assert K.silu_bwd(xv, dyv, out=dx) is dx
        ref, Sc = S.silu_bwd_ref(x, dy)
        E = S.silu_bwd_E(Sc)
        t.count("strays", mem.strays(what), what)
        bad = S.outside(dx, ref, E)
        t.count("outside the interval", int(bad.sum()), f"{what}: x = {x[bad][:6].tolist()}, got {dx.cpu()[bad][:6].tolist()}, ref {ref[bad][:6].tolist()}")
        t.ratio("achieved/E", S.worst_ratio(dx, ref, E), what)
    t.close(note=f"E = {S.FACTOR} x {S.W_SILU_BWD} x 2^-24 |dy| (s + |x| s (1 - s)) (1 + |x| (1 - s)) + 2^-100")


# ------------------------------------------------------------------------------------------------ casts
@pytest.mark.parametrize("scale", S.SCALES)
def test_cast_f32_bf16(K, scale):
    t = Tally(f"cast_f32_bf16 scale={scale:.4f}")
    for n in S.CAST_N:
        for fam in ("edges", "gauss"):
            what = f"n={n} {fam}"
            x = S.edges(n, 1, scale) if fam == "edges" else S.gauss((n,), n, 3.0)
            mem = Mem()
            xv, y = mem.inp(x), mem.out((n,), BF16)
            K.cast_f32_bf16(xv, y, scale)
            ref = S.cast_f32_bf16_ref(x, scale)
            sub = S.cast_subnormals(x, scale)
            t.count("strays", mem.strays(what), what)
            t.exact("mismatches", y, ref, what, mask=~sub)
            t.exact("subnormal mismatches", y, ref, what, mask=sub)
    t.close()


@pytest.mark.parametrize("scale", S.SCALES)
def test_cast_bf16_f32(K, scale):
    t = Tally(f"cast_bf16_f32 scale={scale:.4f}")
    for n in S.CAST_N:
        for fam in ("edges", "gauss"):
            what = f"n={n} {fam}"
            x = S.edges_bf16(n, 1) if fam == "edges" else S.gauss((n,), n, 3.0).to(BF16)
            mem = Mem()
            xv, y = mem.inp(x), mem.out((n,), F32)
            K.cast_bf16_f32(xv, y, scale)
            ref = S.cast_bf16_f32_ref(x, scale)
            sub = S.subnormal_mask(x, ref)
            t.count("strays", mem.strays(what), what)
            t.exact("mismatches", y, ref, what, mask=~sub)
            t.exact("subnormal mismatches", y, ref, what, mask=sub)
    t.close()


# ------------------------------------------------------------------------------------------------ transpose, colsum
@pytest.mark.parametrize("R,C", S.TRANSPOSE)
def test_transpose_and_colsum(K, R, C):
    t = Tally(f"transpose R={R} C={C}")
    ld_in, ld_out = C + 8, R + 8
    xi, f = S.ints(R, C, 9)
    cases = [("ints", xi.to(BF16), S.ints_like((C,), f, 10).to(F32)), ("gauss", S.gauss((R, C), 11).to(BF16), S.gauss((C,), 12)),
             ("edges", S.edges_bf16(R * C, 13).view(R, C), None)]
    forms = dict(ints=("transpose", "transpose+colsum", "colsum"), gauss=("transpose+colsum", "colsum"), edges=("transpose",))
    for fam, x, c0 in cases:
        for form in forms[fam]:
            what = f"{fam} {form}"
            mem = Mem()
            xv = mem.inp(x, ld=ld_in)
            out = mem.out((C, R), BF16, ld=ld_out) if form != "colsum" else None
            cs = mem.acc(c0) if form != "transpose" else None
            if form == "colsum":
                K.colsum(xv, cs)
            else:
                assert K.transpose(xv, out=out, colsum=cs) is out
            t.count("strays", mem.strays(what), what)
            if out is not None:
                t.exact("transpose mismatches", out, S.transpose_ref(x), what)
            if cs is not None:
                ref, A, n = S.colsum_ref(x, c0)
                if fam == "ints":
                    t.exact("colsum mismatches", cs, ref, what)
                else:
                    t.ratio("colsum err/bound", S.sum_ratio(cs, ref, A, n), what)
    t.close()


# ------------------------------------------------------------------------------------------------ cast_transpose
def _up(n, m):
    return (n + m - 1) // m * m


LD_PADS = dict(vector=(0, 0), odd=(1, 1), vector_out_scalar_t=(0, 4), scalar_out_vector_t=(2, 0))   # ld_out % 4 and ld_t % 8 decide, each on its own


def _ct_operands(mem, R, C, ld_in, lds, outputs, seed):
    """w in an arena of row stride ld_in; the shadows in arenas whose every element outside [R, C] / [C, R] - the padding to 128 rows and columns included - is
    NaN: (w, its view, out view or None, out_t view or None)"""
    w = S.edges(R * C, seed).view(R, C)
    wv = mem.inp(w, ld=ld_in)
    ld_out, ld_t = _up(C, 128) + LD_PADS[lds][0], _up(R, 128) + LD_PADS[lds][1]
    out = mem.out((R, C), BF16, ld=ld_out, guard=128) if "out" in outputs else None
    out_t = mem.out((C, R), BF16, ld=ld_t, guard=128) if "out_t" in outputs else None
    return w, wv, out, out_t


@pytest.mark.parametrize("R,C", S.CAST_TRANSPOSE)
def test_cast_transpose(K, R, C):
    t = Tally(f"cast_transpose R={R} C={C}")
    for ld_in in (C, C + 1, _up(C, 4) + 4):
        for lds in LD_PADS:
            for outputs in (("out", "out_t"), ("out",), ("out_t",)):
                what = f"ld_in={ld_in} {lds} {'+'.join(outputs)}"
                mem = Mem()
                w, wv, out, out_t = _ct_operands(mem, R, C, ld_in, lds, outputs, R + C)
                K.cast_transpose(wv, out, out_t)
                o, ot = S.cast_transpose_ref(w)
                t.count("strays", mem.strays(what), what)
                if out is not None:
                    t.exact("out mismatches", out, o, what)
                if out_t is not None:
                    t.exact("out_t mismatches", out_t, ot, what)
    t.close()


@pytest.mark.parametrize("njobs", (1, 6))
def test_cast_transpose_multi(K, njobs):
    """against the statement (not against the single-matrix kernel): one job; six jobs of every shape with missing outputs and a matrix shorter than one tile"""
    t = Tally(f"cast_transpose_multi jobs={njobs}")
    plan = [((67, 67), 68, "odd", ("out", "out_t"))] if njobs == 1 else [
        ((65, 64), 64, "vector", ("out", "out_t")), ((8, 192), 192, "vector", ("out_t",)), ((67, 67), 67, "vector_out_scalar_t", ("out", "out_t")),
        ((130, 520), 524, "vector", ("out",)), ((8, 192), 193, "odd", ("out", "out_t")), ((67, 67), 72, "scalar_out_vector_t", ("out", "out_t"))]
    mem, items, refs = Mem(), [], []
    for i, ((R, C), ld_in, lds, outputs) in enumerate(plan):
        w, wv, out, out_t = _ct_operands(mem, R, C, ld_in, lds, outputs, 100 + i)
        items.append((wv, out, out_t))
        refs.append(S.cast_transpose_ref(w))
    jobs = K.cast_transpose_jobs(items, torch.device(DEV))
    K.cast_transpose_multi(jobs)
    t.count("strays", mem.strays(""), "")
    for i, ((_, out, out_t), (o, ot)) in enumerate(zip(items, refs)):
        if out is not None:
            t.exact("out mismatches", out, o, f"job {i}")
        if out_t is not None:
            t.exact("out_t mismatches", out_t, ot, f"job {i}")
    t.close()


def test_cast_transpose_refuses_misaligned_bases(K):
    """a base pointer one element off is refused wherever the leading dimension selects the vector path - by the entry point, and by cast_transpose_jobs for the
    multi entry - and nothing is launched; with odd leading dimensions (scalar paths) the same views are served, exactly"""
    R, C = 64, 64
    t = Tally("cast_transpose misaligned")

    def shifted(mem, shape, dtype, ld, fill=None):
        """a [rows, cols] view of row stride ld that starts one element behind a 16-byte boundary"""
        rows, cols = shape
        a = G.arena((1, rows * ld + 1), rows * ld + 1, dtype, guard_rows=GUARD, device=DEV)
        mem.arenas.append(a)
        v = a.view[0][1:].view(rows, ld)[:, :cols]
        if fill is not None:
            v.copy_(fill.to(DEV))
        assert v.data_ptr() % 16 == (4 if dtype == F32 else 2)
        return a, v

    w = S.edges(R * C, 7).view(R, C)
    o, ot = S.cast_transpose_ref(w)
    for which in ("in", "out", "out_t"):
        mem = Mem()
        if which == "in":
            _, wv = shifted(mem, (R, C), F32, C, fill=w)
        else:
            wv = mem.inp(w)
        out = shifted(mem, (R, C), BF16, 128)[1] if which == "out" else mem.out((R, C), BF16, ld=128, guard=128)
        out_t = shifted(mem, (C, R), BF16, 128)[1] if which == "out_t" else mem.out((C, R), BF16, ld=128, guard=128)
        with pytest.raises(RuntimeError, match="misaligned"):
            K.cast_transpose(wv, out, out_t)
        with pytest.raises(RuntimeError, match="misaligned"):
            K.cast_transpose_jobs([(wv, out, out_t)], torch.device(DEV))
        torch.cuda.synchronize()
        t.count("elements written by a refused call", int((~is_poison(out)).sum()) + int((~is_poison(out_t)).sum()), which)
        if which != "in":
            K.cast_transpose(wv, None if which == "out" else out, None if which == "out_t" else out_t)      # without the misaligned operand: served
            t.exact("mismatches", out_t if which == "out" else out, ot if which == "out" else o, which + " left out")
    # odd leading dimensions: every path is scalar and the same one-element offsets are fine
    mem = Mem()
    a_w, wv = shifted(mem, (R, C), F32, C + 1, fill=w)
    a_o, out = shifted(mem, (R, C), BF16, 129)
    a_t, out_t = shifted(mem, (C, R), BF16, 129)
    K.cast_transpose(wv, out, out_t)
    K.cast_transpose_multi(K.cast_transpose_jobs([(wv, out, out_t)], torch.device(DEV)))
    torch.cuda.synchronize()
    t.exact("mismatches", out, o, "odd strides, shifted bases: out")
    t.exact("mismatches", out_t, ot, "odd strides, shifted bases: out_t")
    pads = (a_o.view[0][1:].view(R, 129)[:, C:], a_t.view[0][1:].view(C, 129)[:, R:])
    t.count("strays", sum(int((~is_poison(p)).sum()) for p in pads) + int((~is_poison(a_o.view[0][:1])).sum()) + int((~is_poison(a_t.view[0][:1])).sum())
            + sum(G.stray_count(a) for a in (a_w, a_o, a_t)), "odd strides, shifted bases")
    t.close()
