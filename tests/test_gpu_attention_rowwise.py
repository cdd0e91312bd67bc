"""Every attention program against dense fp64 attention, row by row, on adversarial scores, out of NaN-guarded strided buffers.

Programs: the 8-wave forward / dQ / dK-dV of csrc/attention.hip (plain, document mask + doc_ranges, causal, dropout), the wave-specialised dK/dV of
attention_dkv_ws.hip, the generated attention_fwd64 / attention_dq64 / attention_dkv64 (whole blocks, and the balanced walk with its half blocks), and the
split-key decode attention of decode.hip.  Reference, row scales, bounds (2u for O / dV, 3u for dQ / dK, the fp32 dot-product bound for lse2) and the input
families are those of tests/attention_ref64.py; tests/test_attention_ref64.py shows on the CPU that two bf16 flash-attention emulations stay within them.

Buffers: every operand of every call is a row-strided view into ONE arena per dtype that is pre-filled with NaN, with 256 guard rows (a full tile of the
largest program) in front of and behind it inside the same allocation - so nothing here reads or writes outside an allocation.  Two layouts: `separate`
(row stride d + 8, NaN in the 8-element gap) and `engine` (q | k in [M, 2d], v at column 2d of [M, 3d], dq | dk into [M, 2d], dv into columns 2d.. of [M, 3d]).
After each call (a) every element the call owns is finite and within the row bounds, (b) every other arena element is bit-identical (compared as integers).
A key tile past L that is masked by a multiply instead of a select, or a stray store into a stride gap, fails here.

Every bound goes through ledger.check: one ledger row per (path, shape, family, layout, output) with the worst row's error, its (b, h, row) and the bound."""
import pytest
import torch

import attention_ref64 as R
import ledger

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
GUARD = 256
LAYOUTS = ("separate", "engine")
P_DROP, SEED = 0.25, 0x5EED0123456789


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


class Arena:
    """One NaN-filled allocation; `add` reserves [rows, width] with GUARD rows of the same width before and after it."""

    def __init__(self, dtype, device=DEV):
        self.dtype, self.device, self.req = dtype, device, []
        self.ints = torch.int16 if dtype == BF16 else torch.int32

    def add(self, name, rows, width):
        self.req.append((name, rows, width))

    def build(self):
        up = lambda n: (n + 7) // 8 * 8
        self.buf = torch.full((sum(up((rows + 2 * GUARD) * width) for _, rows, width in self.req),), float("nan"), dtype=self.dtype, device=self.device)
        self.owned = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        views, off = {}, 0
        for name, rows, width in self.req:
            views[name] = self.buf[off + GUARD * width: off + (GUARD + rows) * width].view(rows, width)
            off += up((rows + 2 * GUARD) * width)
        return views

    def snapshot(self, *owned):
        """remember every bit; the views in `owned` are what the next call may write"""
        self.snap = self.buf.view(self.ints).clone()
        self.owned.zero_()
        for v in owned:
            self.owned.as_strided(v.size(), v.stride(), v.storage_offset()).fill_(True)

    def stray(self):
        """number of elements outside the owned views whose bits changed since the snapshot (and the first such index)"""
        changed = (self.buf.view(self.ints) != self.snap) & ~self.owned
        n = int(changed.sum())
        return n, (int(changed.nonzero()[0]) if n else -1)


def _flat(t):          # [B, H, L, D] -> [B L, H D]
    B, H, L, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * D)


def _heads(t, B, H, L, D):   # device [B L, H D] view -> CPU fp32 [B, H, L, D]
    return t.float().cpu().reshape(B, L, H, D).permute(0, 2, 1, 3)


def _attention_buffers(layout, B, H, L, D):
    d, M = H * D, B * L
    A, F = Arena(BF16), Arena(F32)
    if layout == "separate":
        for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
            A.add(n, M, d + 8)
    else:
        for n, w in (("qkr", 2 * d), ("qkv", 3 * d), ("o", d), ("do", d), ("dqkr", 2 * d), ("dqkv", 3 * d)):
            A.add(n, M, w)
    F.add("lse", B * H, L)
    F.add("delta", 3 * B * H, L)
    a, f = A.build(), F.build()
    if layout == "separate":
        op = {n: a[n][:, :d] for n in a}
    else:
        op = dict(q=a["qkr"][:, :d], k=a["qkr"][:, d:], v=a["qkv"][:, 2 * d:], o=a["o"], do=a["do"], dq=a["dqkr"][:, :d], dk=a["dqkr"][:, d:], dv=a["dqkv"][:, 2 * d:])
    op["lse"], op["delta"] = f["lse"], f["delta"]
    return A, F, op


def _run_attention(K, layout, q, k, v, do, *, prescaled, causal=False, sample_ids=None, p_drop=0.0, ranges="from_ids"):
    """udm_attention_fwd / _bwd (or the _dropout entry points) on guarded views with explicit strides.  `ranges`: "from_ids" = udm_attention_doc_ranges of the
    sample ids go with them, None = the ids alone (every tile walked, every pair tested).  Returns (dict of CPU outputs [B, H, L, D], list of faults)."""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    B, H, L, D = q.shape
    A, F, op = _attention_buffers(layout, B, H, L, D)
    for n, t in (("q", q), ("k", k), ("v", v), ("do", do)):
        op[n].copy_(_flat(t).to(DEV))
    assert ranges in ("from_ids", None)
    sid = None
    if sample_ids is not None:
        sid = sample_ids.to(DEV)
        ranges = K.attention_doc_ranges(sid) if ranges == "from_ids" else None
    else:
        ranges = None
    flags = (K.ATTN_Q_PRESCALED if prescaled else 0) | (K.ATTN_CAUSAL if causal else 0)
    tail = (float(p_drop), SEED, _s()) if p_drop else (_s(),)
    sfx = "_dropout" if p_drop else ""
    st = lambda n: op[n].stride(0)
    faults = []

    def settle(what):
        torch.cuda.synchronize()
        for name, ar in (("bf16", A), ("fp32", F)):
            n, first = ar.stray()
            if n:
                faults.append(f"{what}: {n} {name} arena elements outside the call's outputs changed (first at flat index {first})")

    A.snapshot(op["o"])
    F.snapshot(op["lse"])
    _lib.call("udm_attention_fwd" + sfx, _p(op["q"]), _p(op["k"]), _p(op["v"]), _p(op["o"]), _p(op["lse"]), _p(sid), _p(ranges), B, H, L, D,
              st("q"), st("k"), st("v"), st("o"), flags, *tail)
    settle("forward")
    A.snapshot(op["dq"], op["dk"], op["dv"])
    F.snapshot(op["delta"])
    _lib.call("udm_attention_bwd" + sfx, _p(op["q"]), _p(op["k"]), _p(op["v"]), _p(op["o"]), _p(op["do"]), _p(op["lse"]), _p(op["delta"]), _p(op["dq"]), _p(op["dk"]),
              _p(op["dv"]), _p(sid), _p(ranges), B, H, L, D, st("q"), st("k"), st("v"), st("o"), st("do"), st("dq"), st("dk"), st("dv"), flags, *tail)
    settle("backward")
    got = {n: _heads(op[n], B, H, L, D) for n in ("o", "dq", "dk", "dv")}
    got["lse2"] = op["lse"].cpu().reshape(B, H, L)
    return got, faults


def _judge(test, tag, got, ref, faults, keys=("o", "dq", "dk", "dv"), dead_rows=None):
    """finite + row bounds + lse2 bound, each through ledger.check; every miss of the case is collected into `faults`"""
    for key in keys:
        if not bool(torch.isfinite(got[key]).all()):
            faults.append(f"{tag} {key}: {int((~torch.isfinite(got[key])).sum())} non-finite elements")
        worst, median, where = R.row_errors(torch.nan_to_num(got[key], nan=float("inf")), ref[key], ref["sc_" + key])
        try:
            ledger.check(test, f"{tag}/{key}", worst, R.BOUNDS[key], note=f"worst row (b, h, row) = {where}; {worst / R.U:.2f} u, median {median / R.U:.2f} u")
        except AssertionError as e:
            faults.append(f"{e} [worst row (b, h, row) = {where}, {worst / R.U:.2f} u, median {median / R.U:.2f} u]")
        if dead_rows is not None and not bool((got[key][dead_rows] == 0).all()):
            faults.append(f"{tag} {key}: padding rows are not exactly 0")
    if "lse2" in got:
        excess, where, dead_ok = R.lse_excess(got["lse2"], ref)
        try:
            ledger.check(test, f"{tag}/lse2 error over its bound", excess, 1.0, note=f"worst row (b, h, row) = {where}")
        except AssertionError as e:
            faults.append(f"{e} [worst row {where}]")
        if not dead_ok:
            faults.append(f"{tag}: lse2 of a row without visible keys is not +inf")


def _case(K, test, tag, family, B, H, L, D, *, prescaled, causal=False, sample_ids=None, p_drop=0.0, configs=((None, None),)):
    """one (shape, family, variant): the fp64 reference once, then every (config name, switch setter) x layout"""
    assert B * H * L * L <= 2.7e7
    q, k, v, do = R.make_inputs(family, B, H, L, D, prescaled=prescaled, causal=causal, sample_ids=sample_ids, seed=1000 * L + D + len(family))
    zt = R.keep_scaled(SEED, P_DROP, B, H, L) if p_drop else None
    ref = R.attention_ref64(q, k, v, do, prescaled=prescaled, sample_ids=sample_ids, causal=causal, zt=zt)
    dead = None if sample_ids is None else (sample_ids == -1)[:, None, :].expand(B, H, L)
    faults = []
    for cname, setter in configs:
        try:
            if setter:
                setter(True)
            for layout in LAYOUTS:
                got, f = _run_attention(K, layout, q, k, v, do, prescaled=prescaled, causal=causal, sample_ids=sample_ids, p_drop=p_drop)
                full = f"{tag}/{B}x{H}x{L}x{D}/{'prescaled' if prescaled else 'plain'}/{family}/{cname + '/' if cname else ''}{layout}"
                faults += [f"{full}: {x}" for x in f]
                _judge(test, full, got, ref, faults, dead_rows=dead)
        finally:
            if setter:
                setter(False)
    assert not faults, "\n".join(faults)


def _switches(K, fwd64=1, dq64=1, dkv64=1, tr=1, cus=0, dkv_ws=1):
    """a setter: (True) puts the debug switches of the library where the test wants them, (False) puts them back: the three program switches and attention_dkv_ws
    to -1 (the library's unset state: the environment's choice, or on), the transposing reads on (the library has no other start value), the CU plan to what it was
    before"""
    before = {}

    def setter(on):
        if on:
            before["cus"] = K._CUS[0]
        K.set_attention_fwd64(fwd64 if on else -1)
        K.set_attention_dq64(dq64 if on else -1)
        K.set_attention_dkv64(dkv64 if on else -1)
        K.debug_set("attention_dkv_ws", dkv_ws if on else -1)
        K.set_tr_read(bool(tr) if on else True)
        K.gemm_set_cus(cus if on else before.get("cus", 0))
    return setter


# ------------------------------------------------------------------------------------------------ 8-wave kernels of attention.hip
@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,H,L,D", [(2, 3, 100, 32), (2, 3, 384, 64), (2, 3, 640, 128), (1, 1, 200, 128)])
def test_generic_8wave(K, B, H, L, D, family, prescaled):
    """attn_fwd_kernel / attn_bwd_dq_kernel / attn_bwd_dkv_kernel without a mask (B H is not a multiple of 8: no generated program takes these shapes; at head dim
    128 dK / dV come from the wave-specialised kernel).  The 384 x 64 and the 640 x 128 shape also run with attention_tr_read = 0: every pass is then the
    USE_TR = false instantiation of its 8-wave kernel - at head dim 128 the single-role dK / dV kernel with the scalar LDS gathers, which is NOT the USE_TR = true
    instantiation that attention_dkv_ws = 0 selects (test_single_role_dkv_d128 has that one)."""
    assert (B * H) % 8 != 0
    configs = [("", _switches(K))]
    if L == 384 or D == 128 and L == 640:
        configs.append(("tr_read0", _switches(K, tr=0)))
    _case(K, "test_generic_8wave", "generic", family, B, H, L, D, prescaled=prescaled, configs=configs)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("layout_name", ["contiguous", "padding"])
@pytest.mark.parametrize("B,H,L,D", [(3, 2, 640, 64), (3, 2, 640, 128)])
def test_document_mask(K, B, H, L, D, layout_name, family, prescaled):
    """sample_ids + doc_ranges: the tile-skipping walks, the per-element id test at document boundaries, document-pure key blocks in the wave-specialised dK/dV
    kernel (head dim 128); rows of padding (id -1) are exactly 0 in O, dQ, dK, dV and hold lse2 = +inf"""
    sid = R.doc_layouts(B, L)[layout_name]
    _case(K, "test_document_mask", f"doc_{layout_name}", family, B, H, L, D, prescaled=prescaled, sample_ids=sid, configs=[("", _switches(K))])


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("B,H,L,D", [(2, 3, 200, 32), (2, 3, 640, 64), (2, 3, 640, 128)])
def test_causal(K, B, H, L, D, family, prescaled):
    """UDM_ATTN_CAUSAL: the triangular walks of the 8-wave kernels (ramp_up moves the exponent on every tile of the walk, up to the diagonal)"""
    _case(K, "test_causal", "causal", family, B, H, L, D, prescaled=prescaled, causal=True, configs=[("", _switches(K))])


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("B,H,L,D", [(4, 2, 320, 128), (4, 3, 200, 64)])
def test_dropout(K, B, H, L, D, family, causal, prescaled):
    """udm_attention_fwd_dropout / _bwd_dropout at p = 0.25, the keep mask restated in tests/attn_prob_dropout_ref.py (the pointer family loses its one key in a
    quarter of the rows: O is then the 2^-20 remainder, which the row scale follows)"""
    _case(K, "test_dropout", "dropout_causal" if causal else "dropout", family, B, H, L, D, prescaled=prescaled, causal=causal, p_drop=P_DROP, configs=[("", _switches(K))])


# ------------------------------------------------------------------------------------------------ generated programs, wave-specialised dK/dV
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,H,L,D", [(1, 8, 768, 128), (2, 4, 1280, 128)])
def test_generated_fwd64_dq64_dkv64(K, B, H, L, D, family):
    """attention_fwd64 / attention_dq64 / attention_dkv64 (head dim 128, q pre-scaled, L % 256 == 0, B H % 8 == 0): switch 1 on the whole chip (24 / 40 blocks, one
    each), switch 1 with 16 CUs planned (24 / 40 blocks = whole rounds + half a grid: the balanced walk with its 128-row half blocks, several blocks per
    persistent workgroup), switch 2 with 16 CUs (the same grid, whole blocks only).  ramp_up moves the reference exponent on every key tile: every return tag of the
    forward's out-of-line rescale block."""
    assert D == 128 and L % 256 == 0 and L >= 512 and (B * H) % 8 == 0 and H >= 2
    nblk = L // 256 * B * H
    assert nblk % 16 == 8 and nblk >= 24      # 16 CUs: rem * 2 == grid, the condition of the balanced walk
    configs = [("switch1", _switches(K, 1, 1, 1)), ("switch1_16cus_halves", _switches(K, 1, 1, 1, cus=16)), ("switch2_16cus", _switches(K, 2, 2, 2, cus=16))]
    _case(K, "test_generated_fwd64_dq64_dkv64", "generated", family, B, H, L, D, prescaled=True, configs=configs)


@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("B,H,L,D,prescaled", [(1, 3, 1000, 128, True), (1, 3, 1000, 128, False), (1, 8, 768, 128, True)])
def test_wave_specialised_dkv(K, B, H, L, D, prescaled, family):
    """attention_dkv_ws.hip: a length that is no multiple of any tile (B H = 3: no generated program), and the generated shape with attention_dkv64 = 0 (the
    generated dQ pass then leaves the planes this kernel starts its score chains from)"""
    configs = [("dkv64_off", _switches(K, 1, 1, 0))]
    _case(K, "test_wave_specialised_dkv", "dkv_ws", family, B, H, L, D, prescaled=prescaled, configs=configs)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
def test_single_role_dkv_d128(K, family, prescaled):
    """attn_bwd_dkv_kernel<128, no ids, USE_TR = true, both accumulators, one wave per SIMD> without a mask: what head dim 128 falls back to when the
    wave-specialised kernel is switched off (attention_dkv_ws = 0, UDM_DKV_WS=0), with a ragged last tile and B H = 3"""
    _case(K, "test_single_role_dkv_d128", "dkv_single", family, 1, 3, 200, 128, prescaled=prescaled, configs=[("dkv_ws0", _switches(K, dkv_ws=0))])


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("family", R.DECODE_FAMILIES)
@pytest.mark.parametrize("p", [65, 1000, 4095])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_decode(K, D, p, family):
    """udm_attention_decode: the cache slots past p hold NaN, the new row is appended into slot p (NaN before), keys are split over workgroups whose running
    maxima differ by hundreds (ramp_up: all the weight in the last split; ramp_down: in the first; pointer: in one key, for one (b, h) the appended one)"""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    B, H = 3, 5
    d, n = H * D, p + 1
    Lmax = 4096 if p == 4095 else p + 64
    q, k, v, _ = R.make_decode_inputs(family, B, H, n, D, seed=7 * p + D)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    A, F = Arena(BF16), Arena(F32)
    for name, rows, w in (("qkr", B, 2 * d), ("qkv", B, 3 * d), ("o", B, d + 8), ("kc", B * Lmax, d), ("vc", B * Lmax, d)):
        A.add(name, rows, w)
    F.add("ws", B * H * 32, D + 2)
    a, ws = A.build(), F.build()["ws"]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, -1, d)       # [B, H, n, D] -> [B, n, H D]
    a["qkr"][:, :d].copy_(rows(q)[:, 0].to(DEV))
    a["qkr"][:, d:].copy_(rows(k)[:, p].to(DEV))
    a["qkv"][:, 2 * d:].copy_(rows(v)[:, p].to(DEV))
    kc, vc = a["kc"].view(B, Lmax, d), a["vc"].view(B, Lmax, d)
    kc[:, :p].copy_(rows(k)[:, :p].to(DEV))
    vc[:, :p].copy_(rows(v)[:, :p].to(DEV))
    o = a["o"][:, :d]
    A.snapshot(o, kc[:, p], vc[:, p])
    F.snapshot(ws)
    _lib.call("udm_attention_decode", _p(a["qkr"][:, :d]), _p(a["qkr"][:, d:]), _p(a["qkv"][:, 2 * d:]), _p(kc), _p(vc), _p(o), _p(ws), ws.numel(), B, H, D, Lmax, p,
              2 * d, 2 * d, 3 * d, d + 8, _s())
    torch.cuda.synchronize()
    faults = []
    for name, ar in (("bf16", A), ("fp32", F)):
        cnt, first = ar.stray()
        if cnt:
            faults.append(f"{cnt} {name} arena elements outside the call's outputs changed (first at flat index {first})")
    if not (torch.equal(kc[:, p].view(torch.int16), a["qkr"][:, d:].view(torch.int16)) and torch.equal(vc[:, p].view(torch.int16), a["qkv"][:, 2 * d:].view(torch.int16))):
        faults.append("cache slot p does not hold the new key / value row")
    got = dict(o=o.float().cpu().reshape(B, 1, H, D).permute(0, 2, 1, 3))
    _judge("test_decode", f"decode/{B}x{H}xD{D}/p{p}/{family}", got, ref, faults, keys=("o",))
    assert not faults, "\n".join(faults)
