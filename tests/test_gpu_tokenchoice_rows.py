"""The token-choice kernels on a real MI355X (pytest -m gpu) against the fp64 reference of tests/tokenchoice_ref64.py: udm_ddpm_sample_rows,
udm_ddpm_sample_rows_cfg, udm_categorical_sample_rows (csrc/ce.hip) and udm_ar_sample_rows (csrc/decode.hip).

Every operand is a view inside a NaN arena with guard rows, and every column a row must not depend on holds NaN: [V, ld), the other modality's ids under
`restrict`, mask_id's logit (except in the greedy form, which states a value for it), the uniforms of every forbidden id (mask_id's own among them in the
categorical forms), and for AR every g column outside
[g_col0, g_col0 + V) and on every inadmissible id.  The `spikes` family keeps finite +80 spikes on its forbidden logits instead.  Per row, none skipped:
    token      in the near-maximum set of the fp64 race; the lowest of ids with bit-identical inputs; id 0 where every score is 0
    undecided  no row, except in `near_tie` where every row is and the token is one of the two constructed ids
    out_logp   |got - ref| <= 2e-4 + 1e-5 |ref| for the drawn and the `given=` token, -inf exactly for a `given` id that is not valid
    w = 0 rows of a guided call equal the unguided call bit for bit; nothing outside the outputs changes
Philox: tokens from `seed=` equal, bit for bit, tokens from the host's uniforms (ddpm, categorical); for AR they satisfy the race rule with the fp64 Gumbel of
the host's grid points and the measured margin, two launches agree, and another step, seed or row changes them.
One ledger row per (entry point, shape, family, form): the shortfall of the worst row against its margin.
"""
import pytest
import torch

import gemm_ref64 as G
import ledger
import nucleus_ref64 as N
import tokenchoice_ref64 as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SENT = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


class IntGuard:
    """an int64 [n] buffer between sentinel guards, itself filled with the sentinel"""

    def __init__(self, n, g=16):
        self.raw = torch.full((n + 2 * g,), SENT, dtype=torch.int64, device=DEV)
        self.view, self.n, self.g = self.raw[g:g + n], n, g

    def untouched(self):
        return bool((self.raw[:self.g] == SENT).all()) and bool((self.raw[self.g + self.n:] == SENT).all())


class Guarded:
    """an integer or bool operand of any shape as a view inside a sentinel-filled buffer of its own kind; intact() holds while the guards and the contents are unchanged"""

    def __init__(self, t, g=64):
        raw_t = t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous()
        fill = 0x5A if raw_t.dtype == torch.uint8 else SENT
        self.raw = torch.full((raw_t.numel() + 2 * g,), fill, dtype=raw_t.dtype, device=DEV)
        self.raw[g:g + raw_t.numel()] = raw_t.reshape(-1).to(DEV)
        self.want = self.raw.clone()
        body = self.raw[g:g + raw_t.numel()].view(raw_t.shape)
        self.view = body.view(torch.bool) if t.dtype == torch.bool else body

    def intact(self):
        return torch.equal(self.raw, self.want)


def _vec(t):
    """a [n] operand as a row of a NaN arena"""
    return G.arena((1, t.numel()), (t.numel() + 3) // 4 * 4, t.dtype, guard_rows=4, device=DEV, fill=t[None])


def _same_bits(a, b):
    iv = torch.int16 if a.dtype == BF16 else torch.int32
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


# ------------------------------------------------------------------------------------------------ ddpm, ddpm_cfg, greedy, categorical
class DdpmOperands:
    def __init__(self, c, form, u=None):
        kind, guided, philox = T.form_of(form)
        M, V, ld = c["M"], c["V"], c["ld"]
        finite = c["family"] == "spikes"
        self.c, self.kind, self.guided = c, kind, guided
        self.pz = N.poison(c["zc"], c["valid"], V, keep_finite=finite)
        if kind == "greedy":
            self.pz[:, c["mask_id"]] = c["zc"][:, c["mask_id"]]             # the greedy form reads mask_id's logit
        self.zc = G.arena((M, ld), ld, BF16, guard_rows=8, device=DEV, fill=self.pz)
        self.zu = self.w = self.u = None
        if guided:
            self.pzu = N.poison(c["zu"], c["valid"], V, keep_finite=finite)
            if kind == "greedy":
                self.pzu[:, c["mask_id"]] = c["zu"][:, c["mask_id"]]
            self.zu = G.arena((M, ld), ld, BF16, guard_rows=8, device=DEV, fill=self.pzu)
            self.w = _vec(c["w"])
        if kind != "greedy":
            uu = c["u"].clone() if u is None else torch.cat([u, torch.zeros(M, ld - V)], 1)
            racing = c["valid"].clone()
            if kind != "cat":
                racing[:, c["mask_id"]] = True                               # [MASK] races with its own u (the categorical draw never looks at it)
            self.pu = N.poison(uu, racing, V)
            self.u = G.arena((M, ld), ld, F32, guard_rows=8, device=DEV, fill=self.pu)
        self.t, self.s = _vec(c["t"]), _vec(c["s"])
        self.modg = Guarded(c["modality"])
        self.mod = self.modg.view
        self.before = {n: getattr(self, n).view.cpu().clone() for n in ("zc", "zu", "w", "u", "t", "s") if getattr(self, n) is not None}

    def check_inputs(self):
        """every operand: guard rows and pad columns untouched, contents bit-identical"""
        for name, was in self.before.items():
            a = getattr(self, name)
            G.assert_untouched(a, name)
            assert _same_bits(a.view.cpu(), was), f"{name} changed"
        assert self.modg.intact(), "modality changed"


def _ddpm_call(K, o, *, guided=None, seed=None, given=None):
    """(token [M], out_logp [M] or None) of the form's entry point, raw C calls on the arenas"""
    from unidisc_amd import _lib

    c = o.c
    M, V, ld = c["M"], c["V"], c["ld"]
    guided = o.guided if guided is None else guided
    out = IntGuard(M)
    pu = None if (seed is not None or o.u is None) else K._p(o.u.view)
    zu, w = (K._p(o.zu.view), K._p(o.w.view)) if guided else (None, None)
    r = 1 if c["restrict"] else 0
    logp = None
    if o.kind == "cat":
        logp = G.arena((1, M), M, F32, guard_rows=4, device=DEV).poison()
        gv = IntGuard(M) if given is not None else None
        if gv is not None:
            gv.view.copy_(given.to(DEV))
        _lib.call("udm_categorical_sample_rows", K._p(o.zc.view), zu, w, ld, K._p(o.mod), pu, ld, seed or 0, K._p(gv.view) if gv is not None else None,
                  K._p(out.view), K._p(logp.view), M, V, c["Vt"], c["mask_id"], r, K._s())
    elif guided:
        _lib.call("udm_ddpm_sample_rows_cfg", K._p(o.zc.view), zu, w, ld, K._p(o.mod), K._p(o.t.view), K._p(o.s.view), pu, ld, seed or 0, K._p(out.view), M, V,
                  c["Vt"], c["mask_id"], r, 1 if o.kind == "greedy" else 0, K._s())
    else:
        _lib.call("udm_ddpm_sample_rows", K._p(o.zc.view), ld, K._p(o.mod), K._p(o.t.view), K._p(o.s.view), pu, ld, seed or 0, K._p(out.view), M, V, c["Vt"],
                  c["mask_id"], r, 1 if o.kind == "greedy" else 0, K._s())
    torch.cuda.synchronize()
    assert out.untouched(), "the token output was written outside its rows"
    if logp is not None:
        G.assert_untouched(logp, "out_logp")
    o.check_inputs()
    return out.view.cpu(), (logp.view[0].cpu() if logp is not None else None)


ENTRY = {"race": "udm_ddpm_sample_rows", "greedy": "udm_ddpm_sample_rows", "cat": "udm_categorical_sample_rows"}


@pytest.mark.parametrize("shape", T.DDPM_SHAPES, ids=lambda s: f"V{s[0]}_mask{s[2]}_{'restrict' if s[3] else 'joint'}")
def test_ddpm_and_categorical_rows(K, shape):
    for sh, family, form in T.ddpm_cases():
        if sh != shape:
            continue
        kind, guided, philox = T.form_of(form)
        c, ref = T.ddpm_ref(sh, family, form)
        tag = f"V{sh[0]}_mask{sh[2]}/{family}/{form}"
        o = DdpmOperands(c, form, ref.u if philox else None)
        tok, logp = _ddpm_call(K, o)
        print(f"{tag}: tokens {tok[:6].tolist()}")
        bad, v = T.violations_ddpm(sh, family, form, tok, logp)
        entry = ENTRY[kind] + ("_cfg" if guided and kind != "cat" else "")
        ledger.check("test_gpu_tokenchoice_rows", f"{entry}/{tag}", v.shortfall, v.bound, note=f"worst row {v.row}; {v.undecided} undecided; {bad[:1]}")
        assert bad == [], f"{tag}: {bad}"
        if philox:                                                           # the seed's tokens are the tokens of the host's uniforms, bit for bit
            t2, l2 = _ddpm_call(K, o, seed=T.PHILOX_SEED)
            assert torch.equal(t2, tok), f"{tag}: Philox tokens differ from the host layout's in {int((t2 != tok).sum())} rows"
            assert l2 is None or _same_bits(l2, logp), tag
            t3, _ = _ddpm_call(K, o, seed=T.PHILOX_SEED + 1)
            assert not torch.equal(t3, tok), f"{tag}: another seed, the same tokens"
        if guided:                                                           # w = 0 rows: the unguided call
            t0, l0 = _ddpm_call(K, o, guided=False)
            z = c["w"] == 0
            assert bool(z.any()) and torch.equal(t0[z], tok[z]), f"{tag}: w = 0 rows differ from the unguided call"
            assert l0 is None or _same_bits(l0[z], logp[z]), tag
        if kind == "cat":                                                    # given=: replay of the draw, an id of the other modality, mask_id, any valid id
            M, V = c["M"], c["V"]
            given = tok.clone()
            given[1::4] = c["mask_id"]
            given[2::4] = torch.where(c["modality"][2::4] == 1, torch.zeros(1, dtype=torch.int64), torch.full((1,), V - 1))
            given[3::4] = torch.stack([c["valid"][r].nonzero()[r % 7, 0] for r in range(3, M, 4)])
            tg, lg = _ddpm_call(K, o, given=given)
            assert torch.equal(tg, given), tag
            ok, err = ref.logp_ok(given, lg)
            assert bool(ok.all()), f"{tag}: log p of given ids off by {err:.3e}; not valid -> {lg[~ok][:4].tolist()}"
            assert _same_bits(lg[0::4], logp[0::4]), f"{tag}: the replayed draw has another log p"
            assert bool(torch.isinf(lg[1::4]).all()) and (not c["restrict"] or bool(torch.isinf(lg[2::4]).all())), tag


def test_ddpm_wrapper_and_zero_score_rows(K):
    """the Python wrappers on the same operands, and the regression of the NaN-u fix: a row whose scores are all 0 gives id 0 although id 0 is forbidden and
    its u holds NaN"""
    sh = T.DDPM_SHAPES[3]
    c, ref = T.ddpm_ref(sh, "mask_wins", "race")
    o = DdpmOperands(c, "race")
    tok, _ = _ddpm_call(K, o)
    img_zero = ref.zero & (c["modality"] == 1)
    assert bool(img_zero.any()) and bool(torch.isnan(o.pu[img_zero, 0]).all()) and bool((tok[img_zero] == 0).all())
    t2 = K.ddpm_sample_rows(o.zc.view, c["V"], c["Vt"], c["mask_id"], t=o.t.view[0], s=o.s.view[0], modality=o.mod, restrict=c["restrict"], u=o.u.view)
    assert torch.equal(t2.cpu(), tok)
    c, ref = T.ddpm_ref(sh, "gauss", "cat_cfg")
    o = DdpmOperands(c, "cat_cfg")
    tok, logp = _ddpm_call(K, o)
    t2, l2 = K.categorical_sample_rows(o.zc.view, c["V"], c["Vt"], c["mask_id"], modality=o.mod, restrict=c["restrict"], u=o.u.view, logits_u=o.zu.view, w=o.w.view[0])
    assert torch.equal(t2.cpu(), tok) and _same_bits(l2.cpu(), logp)


# ------------------------------------------------------------------------------------------------ AR
class ArOperands:
    def __init__(self, c, form):
        _, guided, philox = T.form_of(form)
        R, V, ld = c["M"], c["V"], c["ld"]
        finite = c["family"] == "spikes"
        self.c, self.guided, self.philox = c, guided, philox
        rows2 = 2 * R if guided else R
        both = torch.zeros(rows2, ld, dtype=BF16)
        both[:R] = N.poison(c["zc"], c["valid"], V, keep_finite=finite)
        if guided:
            both[R:] = N.poison(c["zu"], c["valid"], V, keep_finite=finite)
        self.both = both
        self.logits = G.arena((rows2, ld), ld, BF16, guard_rows=8, device=DEV, fill=both)
        self.ldg = T.AR_COL0 + V + 24
        pg = torch.where(c["valid"], c["g"], torch.full_like(c["g"], float("nan")))
        self.g = G.arena((R, V), self.ldg, F32, guard_rows=8, device=DEV, fill=pg, col0=T.AR_COL0)
        self.g_rows = self.g.buf[8 * self.ldg:(8 + R) * self.ldg].view(R, self.ldg)
        self.wa = _vec(torch.full((4,), T.AR_W, dtype=F32))
        self.w = self.wa.view[0]
        self.ints = {n: Guarded(c[n]) for n in ("modmap", "x0", "unmask")}
        self.modmap, self.x0, self.unmask = (self.ints[n].view for n in ("modmap", "x0", "unmask"))
        self.g_before, self.w_before = self.g.view.cpu().clone(), self.wa.view.cpu().clone()

    def run(self, K, *, seed=T.AR_SEED, step=T.AR_STEP, writeback=True):
        """(x[:, pos], next_ids[:R or 2 R]) of one launch; x and next_ids sit between sentinels and must change nowhere else"""
        c = self.c
        R, V = c["M"], c["V"]
        xg, ids = IntGuard(R * T.AR_L), IntGuard(2 * R)
        x = xg.view.view(R, T.AR_L)
        x.fill_(7)
        K.ar_sample_rows(self.logits.view, x, T.AR_POS, V, c["Vt"], c["mask_id"], step=step, modality=self.modmap, restrict=True,
                         g=None if self.philox else self.g_rows, g_col0=T.AR_COL0, seed=seed, x0=self.x0 if writeback else None,
                         x0_unmask=self.unmask if writeback else None, next_ids=ids.view, logits_u=self.logits.view[R:] if self.guided else None,
                         w=self.w if self.guided else None, rows=R)
        torch.cuda.synchronize()
        G.assert_untouched(self.logits, "logits")
        G.assert_untouched(self.g, "g")
        G.assert_untouched(self.wa, "w")
        assert _same_bits(self.logits.view.cpu(), self.both), "the logits changed"
        assert _same_bits(self.g.view.cpu(), self.g_before) and _same_bits(self.wa.view.cpu(), self.w_before), "g or w changed"
        assert all(v.intact() for v in self.ints.values()), "the modality map, x0 or x0_unmask changed"
        assert xg.untouched() and ids.untouched(), "x or next_ids was written outside its rows"
        got = x.cpu()
        other = torch.ones(T.AR_L, dtype=torch.bool)
        other[T.AR_POS] = False
        assert bool((got[:, other] == 7).all()), "another column of x was written"
        nid = ids.view.cpu()
        if not self.guided:
            assert bool((nid[R:] == SENT).all()), "next_ids[R:] was written without guidance"
            nid = nid[:R]
        return got[:, T.AR_POS], nid


@pytest.mark.parametrize("shape", T.AR_SHAPES, ids=lambda s: f"V{s[0]}_mask{s[2]}")
def test_ar_rows(K, shape):
    for sh, family, form in T.ar_cases():
        if sh != shape:
            continue
        _, guided, philox = T.form_of(form)
        c, ref = T.ar_ref(sh, family, form)
        tag = f"V{sh[0]}_mask{sh[2]}/{family}/{form}"
        o = ArOperands(c, form)
        tok, _ = o.run(K, writeback=False)                                   # every position free: the token itself
        print(f"{tag}: tokens {tok[:6].tolist()}")
        xcol, nid = o.run(K)                                                 # kept and free positions
        bad, v = T.violations_ar(sh, family, form, tok, xcol, nid)
        ledger.check("test_gpu_tokenchoice_rows", f"udm_ar_sample_rows/{tag}", v.shortfall, v.bound, note=f"worst row {v.row}; {v.undecided} undecided; {bad[:1]}")
        assert bad == [], f"{tag}: {bad}"
        if philox:
            again, _ = o.run(K, writeback=False)
            assert torch.equal(again, tok), f"{tag}: two launches differ"
            if family == "gauss":
                assert not torch.equal(o.run(K, step=T.AR_STEP + 1, writeback=False)[0], tok), f"{tag}: another step, the same tokens"
                assert not torch.equal(o.run(K, seed=T.AR_SEED + 1, writeback=False)[0], tok), f"{tag}: another seed, the same tokens"
            if family == "flat" and not guided:                              # rows 0, 2, 4, ... hold the same logits and the same valid ids
                assert len(set(tok[::2].tolist())) > 8, f"{tag}: rows with the same logits draw the same token"


# ------------------------------------------------------------------------------------------------ the Gumbel of the Philox path, measured
GRID_SEEDS = ((31, 3, None), (78, 0, (830, 5, 0)), (944, 0, (1441, 9, 2 ** 24 - 1)))      # (seed, step, (row, id, x) of a grid end found by a host search)
OFFSETS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)


def test_gumbel_error_on_the_grid(K):
    """The kernel does not output its Gumbel values, so they are measured through its choices.  Row r holds two admissible ids a < b above a floor of -300:
    a wins iff fl(z_a + g_a) >= fl(z_b + g_b).  The guidance mix with w = 2^-8 turns four bf16 values into z_a - z_b = tau at fp32 resolution (its products
    are exact, so the host knows tau exactly), and tau is stepped around the fp64 value g_b - g_a in units of 2^-24 max(|g_a|, |g_b|, 1): the switch from b to
    a brackets the kernel's g_b - g_a.  The figure per row is the outer end of its bracket, an upper bound of the error of the difference (rounding of the two
    additions included); a is the id whose grid point is nearest an end of the grid, and two seeds place the ends themselves, x = 0 and x = 2^24 - 1."""
    R, V, mask_id, w = 2048, 16, 15, 2.0 ** -8
    rows = torch.arange(R)
    worst = (0.0, None)
    for seed, step, end in GRID_SEEDS:
        x = T.philox_x_ar(seed, step, R, V)
        if end is not None:
            assert int(x[end[0], end[1]]) == end[2]
        a = (x[:, :14] - 2 ** 23).abs().argmax(-1)
        b = a + 1 + (torch.randint(0, 1 << 30, (R,), generator=torch.Generator().manual_seed(seed)) % (14 - a))
        g64 = T.gumbel64(x)
        ga, gb = g64[rows, a], g64[rows, b]
        tau_ref = gb - ga
        unit = 2.0 ** -24 * torch.maximum(torch.maximum(ga.abs(), gb.abs()), torch.ones_like(ga))
        logits = G.arena((2 * R, V), V, BF16, guard_rows=8, device=DEV, fill=torch.full((2 * R, V), -300.0))
        wa = _vec(torch.full((4,), w, dtype=F32))
        wt = wa.view[0]
        lo = torch.full((R,), float("-inf"), dtype=torch.float64)
        hi = torch.full((R,), float("inf"), dtype=torch.float64)
        for k in [0] + [s * o for o in OFFSETS for s in (-1, 1)]:
            tau = tau_ref + k * unit
            cb = (-tau).to(BF16).double()
            db = (((1 + w) * cb + tau) / w).to(BF16).double()
            zb = ((1 + w) * cb - w * db).to(F32).double()
            da = (-(zb + tau) / w).to(BF16).double()
            got_tau = -w * da - zb                                           # z_a - z_b, exactly what the kernel mixes
            zc = torch.full((R, V), -300.0)
            zu = torch.full((R, V), -300.0)
            zc[rows, a], zu[rows, a], zc[rows, b], zu[rows, b] = 0.0, da.float(), cb.float(), db.float()
            logits.view.copy_(torch.cat([zc, zu]).to(BF16))
            xg = IntGuard(R)
            K.ar_sample_rows(logits.view, xg.view.view(R, 1), 0, V, V, mask_id, step=step, seed=seed, logits_u=logits.view[R:], w=wt, rows=R)
            tok = xg.view.cpu()
            assert xg.untouched() and _same_bits(logits.view.cpu(), torch.cat([zc, zu]).to(BF16)), "x was written outside its rows, or the logits changed"
            assert bool(((tok == a) | (tok == b)).all()), "a token outside the two admissible ids: a Gumbel value is not finite or grossly off"
            wins = tok == a
            hi = torch.where(wins, torch.minimum(hi, got_tau), hi)
            lo = torch.where(~wins, torch.maximum(lo, got_tau), lo)
        G.assert_untouched(logits, "logits")
        G.assert_untouched(wa, "w")
        assert float(wa.view[0, 0]) == w
        assert bool((lo < hi).all()), "the choice is not monotone in z_a - z_b"
        open_ = torch.isinf(lo) | torch.isinf(hi)
        assert not bool(open_.any()), f"{int(open_.sum())} rows never switch within 256 units: grossly off, first row {int(open_.nonzero()[0])}, x = {x[int(open_.nonzero()[0])].tolist()}"
        err = torch.maximum((hi - tau_ref).abs(), (lo - tau_ref).abs())
        r = int(err.argmax())
        print(f"seed {seed}: worst error of a Gumbel difference {float(err[r]):.3e} ({float(err[r] / unit[r]):.1f} units) at x_a = {int(x[r, a[r]])}, x_b = {int(x[r, b[r]])}; "
              f"median {float(err.median()):.3e}; x_a from {int(x[rows, a].min())} to {int(x[rows, a].max())}")
        if end is not None:
            print(f"  the grid end x = {end[2]}: error {float(err[end[0]]):.3e}, fp64 Gumbel {float(g64[end[0], end[1]]):.6f}")
            assert int(a[end[0]]) == end[1]
        if float(err[r]) > worst[0]:
            worst = (float(err[r]), (seed, r))
    ledger.check("test_gpu_tokenchoice_rows", "udm_ar_sample_rows/gumbel difference error (GUMBEL_TERM is twice it)", worst[0], T.GUMBEL_TERM / 2, note=f"(seed, row) {worst[1]}")
