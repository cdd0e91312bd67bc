"""udm_attention_fwd_kv_split (csrc/attention_kv.hip: the rectangular forward with the keys split over workgroups and a combine launch) against dense fp64
attention, row by row.

Reference, row scales and bounds (2u per row for O, the fp32 dot-product bound for lse2): tests/attention_ref64.py; tests/test_attention_kv_split_ref64.py shows on
the CPU that the split arithmetic stays within them.  Buffers: the Arena harness of tests/test_gpu_attention_kv_rowwise.py (NaN-filled, 256 guard rows, the engine
and the padded layout), with the fp32 workspace in the fp32 arena too: NaN-filled, guarded, and LONGER than the call needs.  After each call every element of O
(and lse) is finite and within its bound, and every arena element outside O, lse and the first S B H Lq (D + 2) floats of the workspace is bit-identical.
Split counts: forced 2, 3 and 8 and 0 (the plan's choice) on every shape - counts that do not divide the tile count, a ragged tile in the last split, requests
above the tile count ((8, 72) has two tiles) - and a workspace that holds fewer splits than requested."""
import pytest
import torch

import attention_kv_cases as C
import attention_ref64 as R
from test_gpu_attention_kv_rowwise import LAYOUTS, SLACK, _judge, _rows
from test_gpu_attention_rowwise import Arena

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
TEST = "attention_kv_split_rowwise"
WS_COLS = 64          # the workspace is reserved as rows of 64 floats (guard rows of the same width)
WS_EXTRA = 1000       # floats behind what the call may use: they must keep their NaN


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def _buffers(layout, B, H, Lq, Lk, D, ws_floats):
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
    F.add("ws", (ws_floats + WS_EXTRA + WS_COLS - 1) // WS_COLS, WS_COLS)
    a, f = A.build(), F.build()
    rows_q = Lq if layout == "engine" else Lq + 3
    op = dict(q=a["q"].view(B, rows_q, -1)[:, :Lq, :d], k=a["k"].view(B, Lmax, -1)[:, :Lk, :d], v=a["v"].view(B, Lmax, -1)[:, :Lk, :d],
              o=a["o"].view(B, rows_q, -1)[:, :Lq, :d], lse=f["lse"], ws=f["ws"].view(-1))
    return A, F, op


def _call(op, B_, H_, Lq_, Lk_, D_, flags, splits, lse=True, name="udm_attention_fwd_kv_split", **over):
    """the entry point on the views of `op`; `over` replaces single arguments (pointers, strides, shape, ws, ws_elems) by name"""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    a = dict(q=op["q"].data_ptr(), k=op["k"].data_ptr(), v=op["v"].data_ptr(), o=op["o"].data_ptr(), lse=_p(op["lse"]) if lse else None, B=B_, H=H_, Lq=Lq_, Lk=Lk_, D=D_,
             ws=op["ws"].data_ptr(), ws_elems=op["ws"].numel(), splits=splits)
    for n in "qkvo":
        a[n + "_stride"], a[n + "_batch"] = op[n].stride(1), op[n].stride(0)
    a.update(over)
    head = (a["q"], a["k"], a["v"], a["o"], a["lse"], a["B"], a["H"], a["Lq"], a["Lk"], a["D"], a["q_stride"], a["k_stride"], a["v_stride"], a["o_stride"], a["q_batch"],
            a["k_batch"], a["v_batch"], a["o_batch"])
    if name == "udm_attention_fwd_kv":
        _lib.call(name, *head, flags, _s())
    else:
        _lib.call(name, *head, a["ws"], a["ws_elems"], a["splits"], flags, _s())


def _expected_splits(K, B, H, Lq, Lk, D, splits, ws_elems=None):
    """the split count the call runs with (the plan's choice or the request, lowered to the tiles, to 32 and to the workspace) and the floats it may write"""
    S, _ = K.attention_kv_split_plan(B, Lq, Lk, H, D, splits)
    per = B * H * Lq * (D + 2)
    if ws_elems is not None:
        S = max(1, min(S, ws_elems // per))
    return S, (S * per if S > 1 else 0)


def _run(K, layout, q, k, v, *, prescaled, splits, lse=True, ws_elems="all", name="udm_attention_fwd_kv_split"):
    """one call on guarded views.  ws_elems: "all" (the whole reserved workspace), an int (that many floats are offered) or None (the NULL workspace).
    Returns (o CPU fp32 [B, H, Lq, D], lse2 CPU [B, H, Lq] or None, raw bf16 o, faults, S)"""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    full = _expected_splits(K, B, H, Lq, Lk, D, splits)[1]      # what the call needs when the workspace does not limit it
    A, F, op = _buffers(layout, B, H, Lq, Lk, D, full)
    for n, t in (("q", q), ("k", k), ("v", v)):
        op[n].copy_(_rows(t).to(DEV))
    flags = K.ATTN_Q_PRESCALED if prescaled else 0
    over = {}
    if ws_elems is None:
        over, offered = dict(ws=None, ws_elems=0), 0
    elif ws_elems == "all":
        offered = op["ws"].numel()
    else:
        over, offered = dict(ws_elems=ws_elems), ws_elems
    S, may_write = _expected_splits(K, B, H, Lq, Lk, D, splits, offered)
    if name == "udm_attention_fwd_kv":
        S, may_write = 1, 0
    assert may_write + WS_EXTRA <= op["ws"].numel()
    A.snapshot(op["o"])
    F.snapshot(*([op["lse"]] if lse else []), op["ws"][:may_write])
    _call(op, B, H, Lq, Lk, D, flags, splits, lse=lse, name=name, **over)
    torch.cuda.synchronize()
    faults = []
    for nm, ar in (("bf16", A), ("fp32", F)):
        n, first = ar.stray()
        if n:
            faults.append(f"{n} {nm} arena elements outside the call's outputs and workspace changed (first at flat index {first})")
    raw = op["o"].contiguous().cpu()
    o = raw.float().reshape(B, Lq, H, D).permute(0, 2, 1, 3)
    return o, (op["lse"].cpu().reshape(B, H, Lq) if lse else None), raw, faults, S


def _case(K, B, H, Lq, Lk, D, splits_list, families=C.FAMILIES, prescaleds=(True, False), layouts=LAYOUTS, want_split=False):
    faults = []
    for family in families:
        for prescaled in prescaleds:
            q, k, v = C.make_case(family, B, H, Lq, Lk, D, prescaled=prescaled)
            ref = R.attention_ref64(q, k, v, prescaled=prescaled)
            for splits in splits_list:
                for layout in layouts:
                    o, lse2, _, f, S = _run(K, layout, q, k, v, prescaled=prescaled, splits=splits)
                    if want_split and S <= 1:
                        faults.append(f"splits={splits}: the call ran unsplit")
                    tag = f"{B}x{H}x{Lq}x{Lk}x{D}/splits{splits}(S={S})/{'prescaled' if prescaled else 'plain'}/{family}/{layout}"
                    faults += [f"{tag}: {x}" for x in f]
                    _judge(TEST, tag, o, lse2, ref, faults)
    assert not faults, "\n".join(faults)


@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("D", C.HEAD_DIMS)
@pytest.mark.parametrize("Lq,Lk", C.SHAPES)
def test_fwd_kv_split_rows_match_fp64(K, Lq, Lk, D, B):
    _case(K, B, 2, Lq, Lk, D, (2, 3, 8, 0))


def test_fwd_kv_split_mid_size_auto_plan(K):
    """captioning at 1.4 B, batch 1: 32 workgroups unsplit, the plan splits on the real device"""
    B, H, Lq, Lk, D = 1, 16, 256, 1280, 128
    S, n = K.attention_kv_split_plan(B, Lq, Lk, H, D)
    assert S > 1 and n == S * B * H * Lq * (D + 2), (S, n)
    _case(K, B, H, Lq, Lk, D, (0,), want_split=True)


@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_one_split_and_null_workspace_are_the_unsplit_kernel(K, D):
    Lq, Lk = 77, 333
    q, k, v = C.make_case("spikes", 2, 2, Lq, Lk, D, prescaled=True)
    _, lse0, raw0, f0, _ = _run(K, "engine", q, k, v, prescaled=True, splits=0, name="udm_attention_fwd_kv")
    assert not f0, f0
    for kw in (dict(splits=1), dict(splits=8, ws_elems=None), dict(splits=0, ws_elems=None), dict(splits=8, ws_elems=2 * 2 * Lq * (D + 2))):
        _, lse1, raw1, f1, S = _run(K, "engine", q, k, v, prescaled=True, **kw)
        assert S == 1 and not f1, (kw, S, f1)
        assert torch.equal(raw1.view(torch.int16), raw0.view(torch.int16)) and torch.equal(lse1.view(torch.int32), lse0.view(torch.int32)), kw


@pytest.mark.parametrize("D", C.HEAD_DIMS)
def test_two_launches_are_bit_identical_and_lse_is_optional(K, D):
    Lq, Lk = 48, 560
    q, k, v = C.make_case("spikes", 2, 2, Lq, Lk, D, prescaled=True)
    _, lse_a, raw_a, fa, S = _run(K, "engine", q, k, v, prescaled=True, splits=3)
    _, lse_b, raw_b, fb, _ = _run(K, "padded", q, k, v, prescaled=True, splits=3)
    _, none, raw_c, fc, _ = _run(K, "engine", q, k, v, prescaled=True, splits=3, lse=False)      # (the lse rows then belong to nobody: none may change)
    assert S == 3 and not fa and not fb and not fc, (fa, fb, fc)
    assert none is None and bool(torch.isfinite(lse_a).all())
    assert torch.equal(raw_a.view(torch.int16), raw_b.view(torch.int16)) and torch.equal(lse_a.view(torch.int32), lse_b.view(torch.int32))
    assert torch.equal(raw_a.view(torch.int16), raw_c.view(torch.int16))


def test_small_workspace_lowers_the_split_count(K):
    """8 splits asked, room for 3 (and a few floats): the call is the 3-split call, and writes no float behind the third split's partials"""
    B, H, Lq, Lk, D = 2, 2, 48, 560, 64
    per = B * H * Lq * (D + 2)
    q, k, v = C.make_case("ramp_up", B, H, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    o3, lse3, raw3, f3, S3 = _run(K, "engine", q, k, v, prescaled=True, splits=3)
    o8, lse8, raw8, f8, S8 = _run(K, "engine", q, k, v, prescaled=True, splits=8, ws_elems=3 * per + 7)
    assert S3 == 3 and S8 == 3 and not f3 and not f8, (S3, S8, f3, f8)
    assert torch.equal(raw3.view(torch.int16), raw8.view(torch.int16)) and torch.equal(lse3.view(torch.int32), lse8.view(torch.int32))
    faults = []
    _judge(TEST, "small workspace: 8 asked, 3 fit", o8, lse8, ref, faults)
    assert not faults, "\n".join(faults)


def test_fwd_kv_split_argument_errors(K):
    B, H, Lq, Lk, D = 2, 2, 48, 560, 64
    A, F, op = _buffers("engine", B, H, Lq, Lk, D, 8 * B * H * Lq * (D + 2))
    for n in "qkv":
        op[n].zero_()
    A.snapshot()
    F.snapshot()
    pre = K.ATTN_Q_PRESCALED
    bad = [
        ("16-byte aligned", dict(q=op["q"].data_ptr() + 8), pre),
        ("16-byte aligned", dict(k=op["k"].data_ptr() + 2), pre),
        ("16-byte aligned", dict(o=op["o"].data_ptr() + 4), pre),
        ("16-byte aligned", dict(ws=op["ws"].data_ptr() + 4), pre),
        ("multiples of 8", dict(k_stride=op["k"].stride(1) + 4), pre),
        ("multiples of 8", dict(q_stride=op["q"].stride(1) + 1), pre),
        ("multiples of 8", dict(v_batch=op["v"].stride(0) + 4), pre),
        ("multiples of 8", dict(o_batch=op["o"].stride(0) + 2), pre),
        ("unknown flags", dict(), pre | K.ATTN_CAUSAL),      # no causal form
        (">= 1", dict(Lk=0), pre),
        (">= 1", dict(Lq=0), pre),
        ("head_dim", dict(D=48), pre),
        ("unknown flags", dict(), 4),
        (">= 0", dict(splits=-1), pre),
        (">= 0", dict(ws_elems=-8), pre),
    ]
    for msg, over, flags in bad:
        with pytest.raises(RuntimeError, match=msg):
            _call(op, B, H, Lq, Lk, D, flags, over.pop("splits", 4), **over)
    torch.cuda.synchronize()
    assert A.stray()[0] == 0 and F.stray()[0] == 0      # nothing was launched
    _call(op, B, H, Lq, Lk, D, pre, 4)                  # ... and the same views are a valid call
    torch.cuda.synchronize()
    assert bool(torch.isfinite(op["o"].float()).all())


def test_kernels_wrapper_engine_layout(K):
    """K.attention_fwd_kv_split / K.attention_kv_split_ws as the engine calls them: q a column view of [M, 2 d], the cache [B', Lmax, d] with B' > B and Lk < Lmax"""
    B, H, Lq, Lk, D = 2, 2, 77, 333, 64
    d = H * D
    q, k, v = C.make_case("gauss", B, H, Lq, Lk, D, prescaled=True)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    qkr = torch.full((B * Lq, 2 * d), float("nan"), dtype=BF16, device=DEV)
    qkr[:, :d] = _rows(q).reshape(B * Lq, d).to(DEV)
    kc = torch.full((B + 1, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full((B + 1, Lk + 11, d), float("nan"), dtype=BF16, device=DEV)
    kc[1:, :Lk], vc[1:, :Lk] = _rows(k).to(DEV), _rows(v).to(DEV)
    ws = K.attention_kv_split_ws(B, Lq, Lk, H, D, DEV, splits=3)
    assert ws.numel() == 3 * B * H * Lq * (D + 2) and ws.dtype == F32
    assert K.attention_kv_split_plan(B, Lq, Lk, H, D, 40) == (6, 6 * B * H * Lq * (D + 2))      # six key tiles
    faults = []
    for splits in (3, 0):
        o, lse = K.attention_fwd_kv_split(qkr[:, :d], kc[1:], vc[1:], B, Lq, Lk, H, D, q_prescaled=True, want_lse=True, ws=ws, splits=splits)      # (a batch-offset view)
        _judge(TEST, f"wrapper/splits{splits}", o.float().cpu().reshape(B, Lq, H, D).permute(0, 2, 1, 3), lse.cpu(), ref, faults)
    assert not faults, "\n".join(faults)
    with pytest.raises(ValueError):
        K.attention_fwd_kv_split(qkr[:, :d], kc, vc, B, Lq, Lk + 12, H, D, q_prescaled=True, ws=ws)
