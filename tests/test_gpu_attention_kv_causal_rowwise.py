"""udm_attention_fwd_kv_causal (csrc/attention_kv.hip: Lq queries at the LAST Lq of Lk cache slots, query i sees the keys j <= i + (Lk - Lq)) against dense
fp64 attention, row by row.

Reference, row scales and bounds (2u per row for O, the fp32 dot-product bound for lse2): tests/attention_ref64.py with causal=True;
tests/test_attention_kv_causal_ref64.py shows on the CPU that two bf16 flash-attention emulations stay within them on these cases and that the comparator
rejects four mutants of the mask.  Cases: tests/attention_kv_causal_cases.py.

Buffers as in tests/test_gpu_attention_kv_rowwise.py: every operand is a strided view into one NaN-filled allocation per dtype with guard rows around it, in
the two layouts of that module (engine: q as the first d columns of a [B Lq, 2 d] buffer, caches [B, Lmax, H D] with Lmax = Lk + 70; padded: odd row and
batch strides).  Cache slots >= Lk hold NaN.  After each call every element of O (and lse) is finite and within its bound and every other arena element is
bit-identical.

Two exact checks, against udm_attention_fwd_kv on the same views: at Lq = 1 the whole output, and on every case the LAST query row, equal the bidirectional
kernel's bits (O and lse2).  That row sees every key and its block walks the same tiles; the wave's vote on moving the reference exponent is taken on the
tile maxima before the causal mask, so the row runs through the same arithmetic."""
import pytest
import torch

import attention_kv_causal_cases as C
import attention_ref64 as R
import ledger
from test_gpu_attention_rowwise import Arena

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
LAYOUTS = ("engine", "padded")
SLACK = 70   # cache slots behind Lk
TEST = "attention_kv_causal_rowwise"


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


def _call(entry, op, B_, H_, Lq_, Lk_, D_, flags, lse=True, **over):
    """an entry point of the family on the views of `op`; `over` replaces single arguments (pointers, strides, shape) by name"""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    a = dict(q=op["q"].data_ptr(), k=op["k"].data_ptr(), v=op["v"].data_ptr(), o=op["o"].data_ptr(), lse=_p(op["lse"]) if lse else None, B=B_, H=H_, Lq=Lq_, Lk=Lk_, D=D_)
    for n in "qkvo":
        a[n + "_stride"], a[n + "_batch"] = op[n].stride(1), op[n].stride(0)
    a.update(over)
    _lib.call(entry, a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["H"], a["Lq"], a["Lk"], a["D"], a["q_stride"], a["k_stride"], a["v_stride"],
              a["o_stride"], a["q_batch"], a["k_batch"], a["v_batch"], a["o_batch"], flags, _s())


def _run(K, layout, q, k, v, *, prescaled, lse=True, bidirectional_too=False):
    """one causal call on guarded views.  Returns a dict: o (CPU fp32 [B, H, Lq, D]), lse2 (CPU [B, H, Lq] or None), raw (bf16 o [B, Lq, H D]), faults, and with
    bidirectional_too raw_bi / lse2_bi: what udm_attention_fwd_kv then writes into the same views."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    A, F, op = _buffers(layout, B, H, Lq, Lk, D)
    for n, t in (("q", q), ("k", k), ("v", v)):
        op[n].copy_(_rows(t).to(DEV))
    flags = K.ATTN_Q_PRESCALED if prescaled else 0
    A.snapshot(op["o"])
    F.snapshot(*([op["lse"]] if lse else []))
    _call("udm_attention_fwd_kv_causal", op, B, H, Lq, Lk, D, flags, lse=lse)
    torch.cuda.synchronize()
    faults = []
    for name, ar in (("bf16", A), ("fp32", F)):
        n, first = ar.stray()
        if n:
            faults.append(f"{n} {name} arena elements outside the call's outputs changed (first at flat index {first})")
    raw = op["o"].contiguous().cpu()
    out = dict(o=raw.float().reshape(B, Lq, H, D).permute(0, 2, 1, 3), lse2=op["lse"].cpu().reshape(B, H, Lq).clone() if lse else None, raw=raw, faults=faults)
    if bidirectional_too:
        _call("udm_attention_fwd_kv", op, B, H, Lq, Lk, D, flags, lse=lse)
        torch.cuda.synchronize()
        out["raw_bi"] = op["o"].contiguous().cpu()
        out["lse2_bi"] = op["lse"].cpu().reshape(B, H, Lq) if lse else None
    return out


def _judge(tag, o, lse2, ref, faults):
    if not bool(torch.isfinite(o).all()):
        faults.append(f"{tag} o: {int((~torch.isfinite(o)).sum())} non-finite elements")
    worst, median, where = R.row_errors(torch.nan_to_num(o, nan=float("inf")), ref["o"], ref["sc_o"])
    try:
        ledger.check(TEST, f"{tag}/o", worst, R.BOUNDS["o"], note=f"worst row (b, h, row) = {where}; {worst / R.U:.2f} u, median {median / R.U:.2f} u")
    except AssertionError as e:
        faults.append(f"{e} [worst row (b, h, row) = {where}, {worst / R.U:.2f} u, median {median / R.U:.2f} u]")
    if lse2 is not None:
        excess, where, dead_ok = R.lse_excess(lse2, ref)
        try:
            ledger.check(TEST, f"{tag}/lse2 error over its bound", excess, 1.0, note=f"worst row (b, h, row) = {where}")
        except AssertionError as e:
            faults.append(f"{e} [worst row {where}]")
        if not dead_ok or not bool(torch.isfinite(lse2).all()):
            faults.append(f"{tag}: a non-finite lse2 (key 0 is visible to every query: no row is dead)")


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _case(K, B, H, Lq, Lk, D, families=C.FAMILIES, prescaleds=(True, False), layouts=LAYOUTS):
    faults = []
    for family in families:
        for prescaled in prescaleds:
            q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
            ref = R.attention_ref64(q, k, v, prescaled=prescaled, causal=True)
            for layout in layouts:
                tag = f"{B}x{H}x{Lq}x{Lk}x{D}/{'prescaled' if prescaled else 'plain'}/{family}/{layout}"
                r = _run(K, layout, q, k, v, prescaled=prescaled, bidirectional_too=True)
                faults += [f"{tag}: {x}" for x in r["faults"]]
                _judge(tag, r["o"], r["lse2"], ref, faults)
                # the last query row sees every key: the bidirectional kernel's bits (at Lq = 1 that is the whole output)
                if not torch.equal(_bits(r["raw"][:, Lq - 1]), _bits(r["raw_bi"][:, Lq - 1])):
                    n = int((_bits(r["raw"][:, Lq - 1]) != _bits(r["raw_bi"][:, Lq - 1])).sum())
                    faults.append(f"{tag}: {n} elements of the last query row differ from udm_attention_fwd_kv's")
                if not torch.equal(_bits(r["lse2"][:, :, Lq - 1]), _bits(r["lse2_bi"][:, :, Lq - 1])):
                    faults.append(f"{tag}: lse2 of the last query row differs from udm_attention_fwd_kv's")
    assert not faults, "\n".join(faults)


@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES)
def test_fwd_kv_causal_rows_match_fp64(K, Lq, Lk, D):
    _case(K, 2, 2, Lq, Lk, D)


def test_fwd_kv_causal_rows_match_fp64_odd_batch_and_heads(K):
    """B H = 15 is no multiple of 8: the plain tile-major block order instead of the XCD-sequential one"""
    _case(K, 3, 5, 129, 193, 64, families=("gauss", "spikes", "pointer"))


@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_fwd_kv_causal_without_lse_is_bit_identical(K, D):
    Lq, Lk = 77, 333
    q, k, v = C.make_case("spikes", 2, 2, Lq, Lk, D, prescaled=True)
    with_lse = _run(K, "engine", q, k, v, prescaled=True)
    without = _run(K, "engine", q, k, v, prescaled=True, lse=False)      # (the fp32 arena then owns nothing: no lse row may change)
    assert not with_lse["faults"] and not without["faults"], (with_lse["faults"], without["faults"])
    assert without["lse2"] is None and bool(torch.isfinite(with_lse["lse2"]).all())
    assert torch.equal(_bits(with_lse["raw"]), _bits(without["raw"]))


def test_fwd_kv_causal_argument_errors(K):
    B, H, Lq, Lk, D = 2, 2, 48, 560, 64
    A, F, op = _buffers("engine", B, H, Lq, Lk, D)
    for n in "qkv":
        op[n].zero_()
    A.snapshot()
    F.snapshot()
    pre = K.ATTN_Q_PRESCALED
    name = "udm_attention_fwd_kv_causal"
    bad = [
        ("Lk = 47 < Lq = 48", dict(Lk=47), pre),
        ("Lk = 1 < Lq = 48", dict(Lk=1), pre),
        ("unknown flags", dict(), pre | K.ATTN_CAUSAL),      # the entry IS the causal form: the flag of the square kernel is not its
        ("unknown flags", dict(), 4),
        ("unknown flags", dict(), 1 << 20),
        ("16-byte aligned", dict(q=op["q"].data_ptr() + 8), pre),
        ("multiples of 8", dict(k_stride=op["k"].stride(1) + 4), pre),
        (">= 1", dict(Lq=0), pre),
        ("head_dim", dict(D=48), pre),
    ]
    for msg, over, flags in bad:
        with pytest.raises(RuntimeError, match=msg) as e:
            _call(name, op, B, H, Lq, Lk, D, flags, **over)
        assert name + ":" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert A.stray()[0] == 0 and F.stray()[0] == 0      # nothing was launched
    _call(name, op, B, H, Lq, Lk, D, pre)               # ... and the same views are a valid call
    torch.cuda.synchronize()
    assert bool(torch.isfinite(op["o"].float()).all())


def test_kernels_wrapper_engine_layout(K):
    """K.attention_fwd_kv_causal as the engine calls it: q a column view of [M, 2 d], the cache [B, Lmax, d] with Lk < Lmax, against the direct reference"""
    B, H, Lq, Lk, D = 2, 2, 77, 333, 64
    d = H * D
    q, k, v = C.make_case("gauss", B, H, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True, causal=True)
    qkr = torch.full((B * Lq, 2 * d), float("nan"), dtype=BF16, device=DEV)
    qkr[:, :d] = _rows(q).reshape(B * Lq, d).to(DEV)
    kc = torch.full((B, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full((B, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    kc[:, :Lk], vc[:, :Lk] = _rows(k).to(DEV), _rows(v).to(DEV)
    o, lse = K.attention_fwd_kv_causal(qkr[:, :d], kc, vc, B, Lq, Lk, H, D, q_prescaled=True, want_lse=True)
    faults = []
    _judge("wrapper", o.float().cpu().reshape(B, Lq, H, D).permute(0, 2, 1, 3), lse.cpu(), ref, faults)
    assert not faults, "\n".join(faults)
    with pytest.raises(ValueError):
        K.attention_fwd_kv_causal(qkr[:, :d], kc, vc, B, Lq, Lk + 12, H, D, q_prescaled=True)
