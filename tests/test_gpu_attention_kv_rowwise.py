"""udm_attention_fwd_kv (csrc/attention_kv.hip: Lq queries against the first Lk slots of a K / V cache) against dense fp64 attention, row by row.

Reference, row scales, bounds (2u per row for O, the fp32 dot-product bound for lse2) and input families: tests/attention_ref64.py; tests/test_attention_kv_ref64.py
shows on the CPU that two bf16 flash-attention emulations stay within them at these rectangular shapes.  The first Lq rows of the family are the queries.

Buffers (the Arena of tests/test_gpu_attention_rowwise.py): every operand is a strided view into one NaN-filled allocation per dtype with 256 guard rows around
it.  Two layouts:
  engine   q = the first d columns of a [B Lq, 2 d] buffer (the qk-norm output), the caches [B, Lmax, H D] with Lmax = Lk + 70, o [B Lq, d]
  padded   row strides d + 8 (q, o) and d + 16 (caches), batch strides of Lq + 3 and Lmax rows: NaN rows between the samples' queries and outputs
Cache slots >= Lk are never written by the test: they hold NaN, like the stride gaps and the rows between samples.  After each call every element of O (and
lse) is finite and within its bound, and every other arena element is bit-identical - a key tile that overhangs Lk and is masked by a multiply, a query row
>= Lq that is read into a live lane, or a store outside O fails here."""
import pytest
import torch

import attention_kv_cases as C
import attention_ref64 as R
import ledger
from test_gpu_attention_rowwise import Arena

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
LAYOUTS = ("engine", "padded")
SLACK = 70   # cache slots behind Lk


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def _buffers(layout, B, H, Lq, Lk, D):
    d, Lmax = H * D, Lk + SLACK
    A, F = Arena(BF16), Arena(F32)
    if layout == "engine":
        A.add("q", B * Lq, 2 * d)
        A.add("k", B * Lmax, d)
        A.add("v", B * Lmax, d)
        A.add("o", B * Lq, d)
    else:
        A.add("q", B * (Lq + 3), d + 8)
        A.add("k", B * Lmax, d + 16)
        A.add("v", B * Lmax, d + 16)
        A.add("o", B * (Lq + 3), d + 8)
    F.add("lse", B * H, Lq)
    a, f = A.build(), F.build()
    rows_q = Lq if layout == "engine" else Lq + 3
    op = dict(q=a["q"].view(B, rows_q, -1)[:, :Lq, :d], k=a["k"].view(B, Lmax, -1)[:, :Lk, :d], v=a["v"].view(B, Lmax, -1)[:, :Lk, :d],
              o=a["o"].view(B, rows_q, -1)[:, :Lq, :d], lse=f["lse"])
    return A, F, op


def _rows(t):          # [B, H, L, D] -> [B, L, H D]
    B, H, L, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * D)


def _call(op, B_, H_, Lq_, Lk_, D_, flags, lse=True, **over):
    """the entry point on the views of `op`; `over` replaces single arguments (pointers, strides, shape) by name"""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    a = dict(q=op["q"].data_ptr(), k=op["k"].data_ptr(), v=op["v"].data_ptr(), o=op["o"].data_ptr(), lse=_p(op["lse"]) if lse else None, B=B_, H=H_, Lq=Lq_, Lk=Lk_, D=D_)
    for n in "qkvo":
        a[n + "_stride"], a[n + "_batch"] = op[n].stride(1), op[n].stride(0)
    a.update(over)
    _lib.call("udm_attention_fwd_kv", a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["H"], a["Lq"], a["Lk"], a["D"], a["q_stride"], a["k_stride"], a["v_stride"],
              a["o_stride"], a["q_batch"], a["k_batch"], a["v_batch"], a["o_batch"], flags, _s())


def _run(K, layout, q, k, v, *, prescaled, lse=True):
    """one call on guarded views.  Returns (o CPU fp32 [B, H, Lq, D], lse2 CPU [B, H, Lq] or None, raw bf16 o, faults)"""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    A, F, op = _buffers(layout, B, H, Lq, Lk, D)
    for n, t in (("q", q), ("k", k), ("v", v)):
        op[n].copy_(_rows(t).to(DEV))
    flags = K.ATTN_Q_PRESCALED if prescaled else 0
    A.snapshot(op["o"])
    F.snapshot(*([op["lse"]] if lse else []))
    _call(op, B, H, Lq, Lk, D, flags, lse=lse)
    torch.cuda.synchronize()
    faults = []
    for name, ar in (("bf16", A), ("fp32", F)):
        n, first = ar.stray()
        if n:
            faults.append(f"{n} {name} arena elements outside the call's outputs changed (first at flat index {first})")
    raw = op["o"].contiguous().cpu()
    o = raw.float().reshape(B, Lq, H, D).permute(0, 2, 1, 3)
    return o, (op["lse"].cpu().reshape(B, H, Lq) if lse else None), raw, faults


def _judge(test, tag, o, lse2, ref, faults):
    if not bool(torch.isfinite(o).all()):
        faults.append(f"{tag} o: {int((~torch.isfinite(o)).sum())} non-finite elements")
    worst, median, where = R.row_errors(torch.nan_to_num(o, nan=float("inf")), ref["o"], ref["sc_o"])
    try:
        ledger.check(test, f"{tag}/o", worst, R.BOUNDS["o"], note=f"worst row (b, h, row) = {where}; {worst / R.U:.2f} u, median {median / R.U:.2f} u")
    except AssertionError as e:
        faults.append(f"{e} [worst row (b, h, row) = {where}, {worst / R.U:.2f} u, median {median / R.U:.2f} u]")
    if lse2 is not None:
        excess, where, dead_ok = R.lse_excess(lse2, ref)
        try:
            ledger.check(test, f"{tag}/lse2 error over its bound", excess, 1.0, note=f"worst row (b, h, row) = {where}")
        except AssertionError as e:
            faults.append(f"{e} [worst row {where}]")
        if not dead_ok:
            faults.append(f"{tag}: lse2 of a row without visible keys is not +inf")


def _case(K, test, B, H, Lq, Lk, D, families=C.FAMILIES, prescaleds=(True, False), layouts=LAYOUTS):
    faults = []
    for family in families:
        for prescaled in prescaleds:
            q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
            ref = R.attention_ref64(q, k, v, prescaled=prescaled)
            for layout in layouts:
                tag = f"{B}x{H}x{Lq}x{Lk}x{D}/{'prescaled' if prescaled else 'plain'}/{family}/{layout}"
                o, lse2, _, f = _run(K, layout, q, k, v, prescaled=prescaled)
                faults += [f"{tag}: {x}" for x in f]
                _judge(test, tag, o, lse2, ref, faults)
    assert not faults, "\n".join(faults)


@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES)
def test_fwd_kv_rows_match_fp64(K, Lq, Lk, D):
    _case(K, "attention_kv_rowwise", 2, 2, Lq, Lk, D)


def test_fwd_kv_rows_match_fp64_odd_batch_and_heads(K):
    """B H = 15 is no multiple of 8: the plain tile-major block order instead of the XCD-sequential one"""
    _case(K, "attention_kv_rowwise", 3, 5, 129, 193, 64, families=("gauss", "spikes", "pointer"))


@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_fwd_kv_without_lse_is_bit_identical(K, D):
    Lq, Lk = 77, 333
    q, k, v = C.make_case("spikes", 2, 2, Lq, Lk, D, prescaled=True)
    _, lse2, raw_with, f1 = _run(K, "engine", q, k, v, prescaled=True)
    _, none, raw_without, f2 = _run(K, "engine", q, k, v, prescaled=True, lse=False)      # (the fp32 arena then owns nothing: no lse row may change)
    assert not f1 and not f2, (f1, f2)
    assert none is None and bool(torch.isfinite(lse2).all())
    assert torch.equal(raw_with.view(torch.int16), raw_without.view(torch.int16))


def test_fwd_kv_argument_errors(K):
    B, H, Lq, Lk, D = 2, 2, 48, 560, 64
    A, F, op = _buffers("engine", B, H, Lq, Lk, D)
    for n in "qkv":
        op[n].zero_()
    A.snapshot()
    F.snapshot()
    pre = K.ATTN_Q_PRESCALED
    bad = [
        ("16-byte aligned", dict(q=op["q"].data_ptr() + 8), pre),
        ("16-byte aligned", dict(k=op["k"].data_ptr() + 2), pre),
        ("16-byte aligned", dict(o=op["o"].data_ptr() + 4), pre),
        ("multiples of 8", dict(k_stride=op["k"].stride(1) + 4), pre),
        ("multiples of 8", dict(q_stride=op["q"].stride(1) + 1), pre),
        ("multiples of 8", dict(v_batch=op["v"].stride(0) + 4), pre),
        ("multiples of 8", dict(o_batch=op["o"].stride(0) + 2), pre),
        ("unknown flags", dict(), pre | K.ATTN_CAUSAL),      # no causal form
        (">= 1", dict(Lk=0), pre),
        (">= 1", dict(Lq=0), pre),
        ("head_dim", dict(D=48), pre),
        ("unknown flags", dict(), 4),
    ]
    for msg, over, flags in bad:
        with pytest.raises(RuntimeError, match=msg):
            _call(op, B, H, Lq, Lk, D, flags, **over)
    torch.cuda.synchronize()
    assert A.stray()[0] == 0 and F.stray()[0] == 0      # nothing was launched
    _call(op, B, H, Lq, Lk, D, pre)                     # ... and the same views are a valid call
    torch.cuda.synchronize()
    assert bool(torch.isfinite(op["o"].float()).all())


def test_kernels_wrapper_engine_layout(K):
    """K.attention_fwd_kv as the engine calls it: q a column view of [M, 2 d], the cache [B, Lmax, d] with Lk < Lmax, against the direct reference"""
    B, H, Lq, Lk, D = 2, 2, 77, 333, 64
    d = H * D
    q, k, v = C.make_case("gauss", B, H, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    qkr = torch.full((B * Lq, 2 * d), float("nan"), dtype=BF16, device=DEV)
    qkr[:, :d] = _rows(q).reshape(B * Lq, d).to(DEV)
    kc = torch.full((B, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full((B, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    kc[:, :Lk], vc[:, :Lk] = _rows(k).to(DEV), _rows(v).to(DEV)
    o, lse = K.attention_fwd_kv(qkr[:, :d], kc, vc, B, Lq, Lk, H, D, q_prescaled=True, want_lse=True)
    faults = []
    _judge("attention_kv_rowwise", "wrapper", o.float().cpu().reshape(B, Lq, H, D).permute(0, 2, 1, 3), lse.cpu(), ref, faults)
    assert not faults, "\n".join(faults)
    with pytest.raises(ValueError):
        K.attention_fwd_kv(qkr[:, :d], kc, vc, B, Lq, Lk + 12, H, D, q_prescaled=True)
