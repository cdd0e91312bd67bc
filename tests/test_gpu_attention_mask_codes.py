"""The attention kernels under mask codes, row by row against dense fp64 attention, out of NaN-guarded strided buffers.

The sample-id slot of udm_attention_fwd / _bwd carries mask codes (csrc/attention_common.h: id in bits 0-31, key class in bits 32-39, query mask in bits 40-47).  The
engine builds them for modality attention dropout (an ASYMMETRIC mask: text queries see text keys only, per sample) and for model.use_attention_mask (padded keys
get class 4, which no query mask contains - alone, on the modality codes, or on packed sample ids).  tests/attention_ref64.py::code_layouts builds those layouts
(tests/test_attention_mask_codes_ref64.py ties its key-mask arithmetic to the engine's, shows on the CPU that two bf16 flash-attention emulations stay within the
bounds on them, and that a wrong predicate - class bits ignored, mask and class swapped, class 4 visible, only -1 as padding - does not).

Machinery (arenas, layouts, stray-write check, judge, ledger) is that of tests/test_gpu_attention_rowwise.py.  Every case: both arena layouts, finite outputs, the row
bounds 2u (O, dV) / 3u (dQ, dK) and the lse2 bound; a query that sees no key holds lse2 = +inf and exact zeros in O and dQ; a key no query sees (class 4, every key of
the sample whose mask is empty) holds exact zeros in dK and dV - its row scale is 0, so row_errors turns any deviation there into inf as well.
doc_ranges = None is the engine's form and runs everywhere.  doc_ranges from udm_attention_doc_ranges of the codes (defined on the id field, valid under class bits)
runs at head dim 64 and 128: O, lse2 and dQ bit-identical to the None run, dK / dV bit-identical at head dim 64 and within the bounds at head dim 128, where the
ranges report no tile as uniform - so no key block is document-pure and none goes to the wave-specialised half of the dK/dV split."""
import pytest
import torch

import attention_ref64 as R
import test_gpu_attention_rowwise as G

pytestmark = pytest.mark.gpu
TEST = "test_attention_mask_codes"
ALL = (("modality", 72), ("modality", 128), ("keypad", 72), ("modality_keypad", 72), ("modality_keypad", 128), ("docs_keypad", 72))
# D, (B, H, L), layouts: the smallest shapes at which each program still has its seams (a ragged last tile at 200; five key tiles, three query blocks at 320)
SHAPES = [
    (32, (4, 3, 200), (("modality", 72), ("keypad", 72))),
    (64, (4, 2, 320), ALL + (("docs_keypad_neg", 72),)),          # (+ padding ids of -2: the predicate's sign test)
    (128, (4, 2, 320), ALL),                                       # ids select the single-role dK/dV kernel
    (256, (4, 1, 320), (("modality", 72), ("docs_keypad", 72))),   # the dK half / dV half launches
]
CASES = [pytest.param(D, *bhl, layout, Lt, id=f"{D}-{layout}-Lt{Lt}") for D, bhl, layouts in SHAPES for layout, Lt in layouts]


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


def _bits(t):
    return t.contiguous().view(torch.int32)


def _judge(tag, got, ref, faults, dead_q, dead_k):
    G._judge(TEST, tag, got, ref, faults, keys=("o", "dq"), dead_rows=dead_q)
    G._judge(TEST, tag, {n: got[n] for n in ("dk", "dv")}, ref, faults, keys=("dk", "dv"), dead_rows=dead_k)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("D,B,H,L,layout,Lt", CASES)
def test_attention_mask_codes(K, D, B, H, L, layout, Lt, family, prescaled):
    assert B * H * L * L <= 2.7e7
    codes = R.code_layouts(B, L, Lt)[layout]
    q, k, v, do = R.make_inputs(family, B, H, L, D, prescaled=prescaled, sample_ids=codes, seed=1000 * L + D + Lt + len(family))
    ref = R.attention_ref64(q, k, v, do, prescaled=prescaled, sample_ids=codes)
    ok = R.pair_ok(codes)
    dead_q, dead_k = ((~ok.any(dim))[:, None, :].expand(B, H, L) for dim in (2, 1))
    assert torch.equal(torch.isinf(ref["lse2"]), dead_q)
    configs = [("", G._switches(K))]
    if D in (64, 128) and (layout, Lt) == ("modality_keypad", 72):
        configs.append(("tr_read0", G._switches(K, tr=0)))       # the USE_TR = false instantiations with ids
    faults = []
    for cname, setter in configs:
        try:
            setter(True)
            for arena in G.LAYOUTS:
                tag = f"codes_{layout}_Lt{Lt}/{B}x{H}x{L}x{D}/{'prescaled' if prescaled else 'plain'}/{family}/{cname + '/' if cname else ''}{arena}"
                got, f = G._run_attention(K, arena, q, k, v, do, prescaled=prescaled, sample_ids=codes, ranges=None)
                faults += [f"{tag}: {x}" for x in f]
                _judge(tag, got, ref, faults, dead_q, dead_k)
                if D not in (64, 128) or cname:
                    continue
                ranges = K.attention_doc_ranges(codes.to(G.DEV)).cpu()
                if not (bool((ranges[..., 2] == -1).all()) and bool((ranges[..., 4] == 0).all())):
                    faults.append(f"{tag}: doc_ranges of codes report a uniform or exact tile (a document-pure block would take the wave-specialised dK/dV kernel)")
                got_r, f = G._run_attention(K, arena, q, k, v, do, prescaled=prescaled, sample_ids=codes, ranges="from_ids")
                faults += [f"{tag}/ranges: {x}" for x in f]
                for name in ("o", "lse2", "dq") + (("dk", "dv") if D == 64 else ()):
                    if not torch.equal(_bits(got_r[name]), _bits(got[name])):
                        faults.append(f"{tag}/ranges: {name} is not bit-identical to the run without doc_ranges ({int((_bits(got_r[name]) != _bits(got[name])).sum())} elements)")
                _judge(tag + "/ranges", got_r, ref, faults, dead_q, dead_k)
        finally:
            setter(False)
    assert not faults, "\n".join(faults)
