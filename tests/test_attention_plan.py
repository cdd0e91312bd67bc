"""Which attention program runs: unidisc_amd/csrc/attention_plan.h, compiled alone with a host compiler (tests/attention_plan_print.cpp) and asked for the plan of
every (shape, switches) combination of the GPU tests that call the attention entry points themselves - tests/test_gpu_attention_rowwise.py, _causal.py, _d256.py,
_prob_dropout.py, _fwd64.py, _dkv64.py and the attention tests of tests/test_gpu_kernels.py - so that a test which believes it exercises one program fails HERE
when a gate moves it onto another; and of one case on each side of every gate (two gates cannot be reached alone: see "NOT covered" below).  The model-level tests
(e2e, AR, sampler) reach attention through the engine at the shapes of their goldens and are not listed.  Expected programs and grid numbers are written out below,
not computed from the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W8 = ("FWD_8WAVE", "DQ_8WAVE")
GEN = ("FWD_GEN64", "DQ_GEN64", "DKV_GEN64")


def _layouts(d):
    """row strides (q k v o do dq dk dv, O of the forward call) of the two layouts of tests/test_gpu_attention_rowwise.py"""
    return dict(separate=(d + 8,) * 9, engine=(2 * d, 2 * d, 3 * d, d, d, 2 * d, 2 * d, 3 * d, d))


CASES = []   # (name, input line without the name, expected)


def case(name, B, H, L, D, expect, *, prescaled=False, sid=False, ranges=False, causal=False, p_drop=0.0, strides=None, sw=(1, 1, 1), dkv_ws=1, dkv_pre=1, tr=1, dev_cus=256,
         plan_cus=0, grids=None):
    """expect = (forward, dQ, dK/dV program, planes_needed); grids = {"fwd_grid" | "dq_grid" | "dkv_grid": (grid, nfull, hashalf[, mg_nt, mg_H])}, or one tuple for all three
    generated programs.  Without `strides` the case runs in both layouts of the GPU tests."""
    if isinstance(grids, tuple):
        grids = {k: grids for k in ("fwd_grid", "dq_grid", "dkv_grid")}
    for lname, st in (_layouts(H * D).items() if strides is None else [("", strides)]):
        nums = (D, B, H, L, int(sid), int(ranges), int(causal), int(prescaled), repr(float(p_drop))) + tuple(st) + tuple(sw) + (dkv_ws, dkv_pre, tr, dev_cus, plan_cus)
        CASES.append((f"{name}/{lname}".rstrip("/").replace(", ", "x").replace("(", "").replace(")", "").replace(" ", "_"), " ".join(str(x) for x in nums), (expect, grids or {})))


for pre in (True, False):
    ws = "DKV_WS_PRE" if pre else "DKV_WS"
    tag = "prescaled" if pre else "plain"
    # ---- tests/test_gpu_attention_rowwise.py
    for shape in ((2, 3, 100, 32), (2, 3, 384, 64)):
        case(f"generic {shape} {tag}", *shape, W8 + ("DKV_SINGLE", False), prescaled=pre)
    case(f"generic 384x64 tr_read0 {tag}", 2, 3, 384, 64, W8 + ("DKV_SINGLE", False), prescaled=pre, tr=0)
    for shape in ((2, 3, 640, 128), (1, 1, 200, 128)):
        case(f"generic {shape} {tag}", *shape, W8 + (ws, pre), prescaled=pre)
    case(f"generic 640x128 tr_read0 {tag}", 2, 3, 640, 128, W8 + ("DKV_SINGLE", False), prescaled=pre, tr=0)
    case(f"generic 640x128 dkv_ws0 {tag}", 2, 3, 640, 128, W8 + ("DKV_SINGLE", False), prescaled=pre, dkv_ws=0)
    case(f"single_role_dkv_d128 {tag}", 1, 3, 200, 128, W8 + ("DKV_SINGLE", False), prescaled=pre, dkv_ws=0)
    case(f"document_mask 640x128 {tag}", 3, 2, 640, 128, W8 + ("DKV_WS_SPLIT_SINGLE", pre), prescaled=pre, sid=True, ranges=True)
    case(f"document_mask 640x128 no ranges {tag}", 3, 2, 640, 128, W8 + ("DKV_SINGLE", False), prescaled=pre, sid=True)
    case(f"document_mask 640x64 {tag}", 3, 2, 640, 64, W8 + ("DKV_SINGLE", False), prescaled=pre, sid=True, ranges=True)
    for shape in ((2, 3, 200, 32), (2, 3, 640, 64), (2, 3, 640, 128)):
        case(f"causal {shape} {tag}", *shape, W8 + ("DKV_SINGLE", False), prescaled=pre, causal=True)
    # tests/test_gpu_attention_causal.py (contiguous rows): never a generated program nor the wave-specialised kernel, (2, 2, 384, 128) and (8, 16, 1280, 128) included
    for shape in [(2, 3, L, D) for D in (32, 64, 128) for L in (128, 384, 1280, 200, 1000)] + [(2, 2, 384, D) for D in (32, 64, 128)] + [(8, 16, 1280, 128), (8, 12, 1280, 64), (1, 2, 128, 64)]:
        case(f"causal torch {shape} {tag}", *shape, W8 + ("DKV_SINGLE", False), prescaled=pre, causal=True, strides=(shape[1] * shape[3],) * 9)
    for causal in (False, True):
        for p in (0.25, 0.1):   # (p = 0.1, the 130 x 32 and the 1280 x 128 shape: test_gpu_attention_prob_dropout.py)
            for shape in ((4, 2, 320, 128), (4, 3, 200, 64), (4, 2, 130, 32), (1, 16, 1280, 128)):
                case(f"dropout p={p} {shape} causal{int(causal)} {tag}", *shape, W8 + ("DKV_SINGLE", False), prescaled=pre, causal=causal, p_drop=p)
    case(f"wave_specialised_dkv 1000 {tag}", 1, 3, 1000, 128, W8 + (ws, pre), prescaled=pre, sw=(1, 1, 0))
    # ---- head dim 256 (tests/test_gpu_attention_d256.py, test_gpu_rowops_d256.py): the dK half and the dV half, whatever else
    for shape in ((2, 3, 100, 256), (1, 3, 320, 256), (1, 8, 256, 256), (1, 8, 768, 256)):
        case(f"d256 {shape} {tag}", *shape, W8 + ("DKV_HALVES_D256", False), prescaled=pre)
    case(f"d256 tr_read0 {tag}", 1, 3, 320, 256, W8 + ("DKV_HALVES_D256", False), prescaled=pre, tr=0)
    case(f"d256 document_mask {tag}", 3, 2, 320, 256, W8 + ("DKV_HALVES_D256", False), prescaled=pre, sid=True, ranges=True)
    for shape in ((2, 3, 200, 256), (1, 2, 384, 256)):
        case(f"d256 causal {shape} {tag}", *shape, W8 + ("DKV_HALVES_D256", False), prescaled=pre, causal=True)
    for causal in (False, True):
        case(f"d256 dropout causal{int(causal)} {tag}", 2, 3, 200, 256, W8 + ("DKV_HALVES_D256", False), prescaled=pre, causal=causal, p_drop=0.25)

# ---- the attention tests of tests/test_gpu_kernels.py (contiguous rows, B = 2 unless said)
def _contig(name, B, H, L, D, expect, **kw):
    case(name, B, H, L, D, expect, strides=(H * D,) * 9, **kw)


for D, H in ((32, 2), (64, 3), (128, 2)):
    for L in (32, 100, 384):
        for tr in (1, 0):
            _contig(f"kernels fwd_bwd {D}x{H}x{L} tr{tr}", 2, H, L, D, W8 + ("DKV_WS" if D == 128 and tr else "DKV_SINGLE", False), tr=tr)
            _contig(f"kernels fwd_bwd {D}x{H}x{L} tr{tr} ids", 2, H, L, D, W8 + ("DKV_SINGLE", False), tr=tr, sid=True)
_contig("kernels prescaled 32x2x100", 2, 2, 100, 32, W8 + ("DKV_SINGLE", False), prescaled=True)
_contig("kernels prescaled 64x3x384 ids", 2, 3, 384, 64, W8 + ("DKV_SINGLE", False), prescaled=True, sid=True)
_contig("kernels prescaled 128x2x384", 2, 2, 384, 128, W8 + ("DKV_WS_PRE", True), prescaled=True)
_contig("kernels prescaled 128x8x512", 2, 8, 512, 128, GEN + (True,), prescaled=True, grids=(32, 32, 0))
_contig("kernels prescaled 128x3x200 ids", 2, 3, 200, 128, W8 + ("DKV_SINGLE", False), prescaled=True, sid=True)
for L in (2, 31, 33, 64, 65, 127, 129, 191, 193, 257, 640, 1000):
    for B, H in ((1, 1), (3, 5)):
        _contig(f"kernels ragged {B}x{H}x{L}", B, H, L, 128, W8 + ("DKV_WS", False))
for D, H in ((64, 3), (128, 2)):
    for L in (100, 640, 1500):
        _contig(f"kernels tile_skipping {D}x{L} ids", 3, H, L, D, W8 + ("DKV_SINGLE", False), sid=True)
        _contig(f"kernels tile_skipping {D}x{L} ids ranges", 3, H, L, D, W8 + ("DKV_WS_SPLIT_SINGLE" if D == 128 else "DKV_SINGLE", False), sid=True, ranges=True)

case("causal 768 prescaled", 1, 8, 768, 128, W8 + ("DKV_SINGLE", False), prescaled=True, causal=True)
# A p_drop that rounds to thr == 0 (attn_drop_thr, which the printer applies as the entry points do; thr = (uint32)(p 65536 + 0.5)) is the call without dropout, the
# generated programs included: p = 0, 1e-6 and the last float below 2^-17; at 2^-17 (thr = 1) the dropout kernels run
for p in (0.0, 1e-6, 7.62939e-06):
    case(f"dropout p={p} 1x16x1280", 1, 16, 1280, 128, GEN + (True,), prescaled=True, p_drop=p, grids=(80, 80, 0))
    case(f"dropout p={p} 4x3x200x64", 4, 3, 200, 64, W8 + ("DKV_SINGLE", False), p_drop=p)
case("dropout p=2^-17 1x16x1280", 1, 16, 1280, 128, W8 + ("DKV_SINGLE", False), prescaled=True, p_drop=2.0 ** -17)
# ---- the generated programs (test_generated_fwd64_dq64_dkv64, tests/test_gpu_attention_fwd64.py, tests/test_gpu_attention_dkv64.py): magic(3) = 1431655766,
# magic(5) = 858993460, magic(4) = 1073741825, magic(8) = 536870913, magic(16) = 268435457 (2^32 / d + 1)
case("generated 768 switch1", 1, 8, 768, 128, GEN + (True,), prescaled=True, grids=(24, 24, 0, 1431655766, 536870913))
case("generated 768 switch1 16cus", 1, 8, 768, 128, GEN + (True,), prescaled=True, plan_cus=16, grids=(16, 16, 1, 1431655766, 536870913))
case("generated 768 switch2 16cus", 1, 8, 768, 128, GEN + (True,), prescaled=True, plan_cus=16, sw=(2, 2, 2), grids=(16, 24, 0, 1431655766, 536870913))
case("generated 1280 switch1", 2, 4, 1280, 128, GEN + (True,), prescaled=True, grids=(40, 40, 0, 858993460, 1073741825))
case("generated 1280 switch1 16cus", 2, 4, 1280, 128, GEN + (True,), prescaled=True, plan_cus=16, grids=(16, 32, 1, 858993460, 1073741825))
case("generated 1280 switch2 16cus", 2, 4, 1280, 128, GEN + (True,), prescaled=True, plan_cus=16, sw=(2, 2, 2), grids=(16, 40, 0, 858993460, 1073741825))
case("headline 8x16x1280 256 CUs", 8, 16, 1280, 128, GEN + (True,), prescaled=True, grids=(256, 512, 1, 858993460, 268435457))
case("headline 8x16x1280 switch2", 8, 16, 1280, 128, GEN + (True,), prescaled=True, sw=(2, 2, 2), grids=(256, 640, 0))
for shape, g in (((1, 8, 512), (16, 16, 0)), ((2, 4, 768), (24, 24, 0)), ((1, 8, 1024), (32, 32, 0)), ((3, 8, 1280), (120, 120, 0)), ((1, 16, 2048), (128, 128, 0)), ((2, 24, 512), (96, 96, 0))):
    case(f"generated {shape}", *shape, 128, GEN + (True,), prescaled=True, grids=g)
# tests/test_gpu_attention_fwd64.py and tests/test_gpu_attention_dkv64.py (contiguous rows): every shape with the switch settings the tests go through - all on,
# fwd64 = 0, dq64 = dkv64 = 0, dq64 = 1 with dkv64 = 0.  384 blocks of 16 tiles: a whole round + halves; 64 blocks: fewer than CUs; no generated program for
# B H = 6, for one head, for L = 256
for shape, g in (((1, 8, 512), (16, 16, 0)), ((2, 4, 768), (24, 24, 0)), ((1, 8, 1024), (32, 32, 0)), ((3, 8, 1280), (120, 120, 0)), ((8, 16, 1280), (256, 512, 1)), ((1, 16, 2048), (128, 128, 0)),
                 ((2, 24, 512), (96, 96, 0)), ((1, 24, 4096), (256, 256, 1)), ((4, 8, 512), (64, 64, 0)), ((2, 3, 512), None), ((8, 1, 512), None), ((1, 8, 256), None)):
    st = (shape[1] * 128,) * 9
    on = g is not None
    case(f"fwd64_dkv64 {shape} all on", *shape, 128, GEN + (True,) if on else W8 + ("DKV_WS_PRE", True), prescaled=True, strides=st, grids=g)
    case(f"fwd64_dkv64 {shape} fwd64=0", *shape, 128, ("FWD_8WAVE", "DQ_GEN64", "DKV_GEN64", True) if on else W8 + ("DKV_WS_PRE", True), prescaled=True, strides=st, sw=(0, 1, 1),
         grids=dict(dq_grid=g, dkv_grid=g) if on else None)
    case(f"fwd64_dkv64 {shape} dq64=dkv64=0", *shape, 128, ("FWD_GEN64" if on else "FWD_8WAVE", "DQ_8WAVE", "DKV_WS_PRE", True), prescaled=True, strides=st, sw=(1, 0, 0),
         grids=dict(fwd_grid=g) if on else None)
    case(f"fwd64_dkv64 {shape} dkv64=0", *shape, 128, ("FWD_GEN64", "DQ_GEN64", "DKV_WS_PRE", True) if on else W8 + ("DKV_WS_PRE", True), prescaled=True, strides=st, sw=(1, 1, 0),
         grids=dict(fwd_grid=g, dq_grid=g) if on else None)
# test_generated_attention_programs_respect_the_cu_plan: at 224 CUs the 640 blocks are no longer whole rounds + half a grid
case("headline 8x16x1280 224 CUs", 8, 16, 1280, 128, GEN + (True,), prescaled=True, strides=(2048,) * 9, plan_cus=224, grids=(224, 640, 0, 858993460, 268435457))
# the engine-layout tests of both files: (2, 4, 1280, 128) with the generated programs on and off
case("engine 2x4x1280 all off", 2, 4, 1280, 128, W8 + ("DKV_WS_PRE", True), prescaled=True, sw=(0, 0, 0))
case("engine 2x4x1280 fwd64=0", 2, 4, 1280, 128, ("FWD_8WAVE", "DQ_GEN64", "DKV_GEN64", True), prescaled=True, sw=(0, 1, 1), grids=dict(dq_grid=(40, 40, 0), dkv_grid=(40, 40, 0)))
case("engine 2x4x1280 dq64=dkv64=0", 2, 4, 1280, 128, ("FWD_GEN64", "DQ_8WAVE", "DKV_WS_PRE", True), prescaled=True, sw=(1, 0, 0), grids=dict(fwd_grid=(40, 40, 0)))
# every planes reader's shape with plain q: the reader is not chosen (the assertion of attn_plan_bwd would abort the printer otherwise)
case("768 plain dkv64 off", 1, 8, 768, 128, W8 + ("DKV_WS", False), sw=(1, 1, 0))
case("768 plain sample ids", 1, 8, 768, 128, W8 + ("DKV_WS_SPLIT_SINGLE", False), sid=True, ranges=True)
case("wave_specialised_dkv 768 dkv64 off", 1, 8, 768, 128, ("FWD_GEN64", "DQ_GEN64", "DKV_WS_PRE", True), prescaled=True, sw=(1, 1, 0), grids=dict(fwd_grid=(24, 24, 0), dq_grid=(24, 24, 0)))
case("768 dq64 off dkv64 on", 1, 8, 768, 128, ("FWD_GEN64", "DQ_8WAVE", "DKV_GEN64", True), prescaled=True, sw=(1, 0, 1), grids=dict(fwd_grid=(24, 24, 0), dkv_grid=(24, 24, 0)))
case("768 all three off", 1, 8, 768, 128, W8 + ("DKV_WS_PRE", True), prescaled=True, sw=(0, 0, 0))
case("768 all off dkv_pre0", 1, 8, 768, 128, W8 + ("DKV_WS", False), prescaled=True, sw=(0, 0, 0), dkv_pre=0)
case("768 all off dkv_ws0", 1, 8, 768, 128, W8 + ("DKV_SINGLE", False), prescaled=True, sw=(0, 0, 0), dkv_ws=0)
case("768 tr_read0", 1, 8, 768, 128, W8 + ("DKV_SINGLE", False), prescaled=True, tr=0)
case("768 sample ids", 1, 8, 768, 128, W8 + ("DKV_WS_SPLIT_SINGLE", True), prescaled=True, sid=True, ranges=True)
# ---- the gate edges, from (1, 8, 768, 128) pre-scaled (all three generated)
FALLBACK = W8 + ("DKV_WS_PRE", True)
case("edge L=256", 1, 8, 256, 128, FALLBACK, prescaled=True)
case("edge L=640", 1, 8, 640, 128, FALLBACK, prescaled=True)
case("edge H=1 B=8", 8, 1, 512, 128, FALLBACK, prescaled=True)
case("edge BH=12", 1, 12, 768, 128, FALLBACK, prescaled=True)
case("edge BH=6", 2, 3, 512, 128, FALLBACK, prescaled=True)
case("edge not prescaled", 1, 8, 768, 128, W8 + ("DKV_WS", False))
d = 8 * 128
S = [d] * 9   # q k v o do dq dk dv, O of the forward


def strided(**kw):
    idx = dict(q=0, k=1, v=2, o=3, do=4, dq=5, dk=6, dv=7, fwd_o=8)
    s = list(S)
    for k, v in kw.items():
        s[idx[k]] = v
    return tuple(s)


G24 = (24, 24, 0)
case("edge contiguous", 1, 8, 768, 128, GEN + (True,), prescaled=True, strides=strided(), grids=G24)
case("edge forward O stride d+4", 1, 8, 768, 128, ("FWD_8WAVE", "DQ_GEN64", "DKV_GEN64", True), prescaled=True, strides=strided(fwd_o=d + 4), grids=dict(dq_grid=G24, dkv_grid=G24))
case("edge dQ stride d+4", 1, 8, 768, 128, ("FWD_GEN64", "DQ_8WAVE", "DKV_GEN64", True), prescaled=True, strides=strided(dq=d + 4), grids=dict(fwd_grid=G24, dkv_grid=G24))
case("edge dK stride d+4", 1, 8, 768, 128, ("FWD_GEN64", "DQ_GEN64", "DKV_WS_PRE", True), prescaled=True, strides=strided(dk=d + 4), grids=dict(fwd_grid=G24, dq_grid=G24))
case("edge dV stride d+4", 1, 8, 768, 128, ("FWD_GEN64", "DQ_GEN64", "DKV_WS_PRE", True), prescaled=True, strides=strided(dv=d + 4), grids=dict(fwd_grid=G24, dq_grid=G24))
# 32-bit lane offsets, 2^31 bytes: q over 256 rows in the forward and dQ (stride 2^22) but over 64 rows in dK/dV; k over 80 rows in the forward (13421776 * 160 >= 2^31),
# 64 in dQ, 256 in dK/dV
case("edge q stride 2^22 - 8", 1, 8, 768, 128, GEN + (True,), prescaled=True, strides=strided(q=(1 << 22) - 8), grids=G24)
case("edge q stride 2^22", 1, 8, 768, 128, W8 + ("DKV_GEN64", True), prescaled=True, strides=strided(q=1 << 22), grids=dict(dkv_grid=G24))
case("edge k stride 80 rows", 1, 8, 768, 128, ("FWD_8WAVE", "DQ_GEN64", "DKV_WS_PRE", True), prescaled=True, strides=strided(k=13421776), grids=dict(dq_grid=G24))
case("edge k stride 2^24", 1, 8, 768, 128, FALLBACK, prescaled=True, strides=strided(k=1 << 24))
case("edge v stride 2^22", 1, 8, 768, 128, ("FWD_GEN64", "DQ_GEN64", "DKV_WS_PRE", True), prescaled=True, strides=strided(v=1 << 22), grids=dict(fwd_grid=G24, dq_grid=G24))
# B H L = 2^29 (lse / plane indices): 512 x 8 x 131072; one block of rows less is taken (2093056 blocks = 8176 whole rounds of 256)
case("edge BHL 2^29 - 1 block row", 512, 8, 131072 - 256, 128, GEN + (True,), prescaled=True, strides=strided(), grids=(256, 2093056, 0))
case("edge BHL 2^29", 512, 8, 131072, 128, FALLBACK, prescaled=True, strides=strided())
# NOT covered: the gates B L >= 2^30 and blocks >= 2^24.  Neither can be reached below B H L = 2^29 (H >= 2, 256 rows per block), so these two cases fall back on
# the plane limit already and would stay green with either gate deleted; the gates are kept as the launchers had them
case("edge BL 2^30", 1 << 20, 2, 1024, 128, FALLBACK, prescaled=True, strides=strided())
case("edge 2^24 blocks", 4096, 8, 131072, 128, FALLBACK, prescaled=True, strides=strided())
# magic divisions: L / 256 <= 4096, H <= 4096
case("edge L/256 = 4096", 1, 8, 4096 * 256, 128, GEN + (True,), prescaled=True, strides=strided(), grids=(256, 32768, 0))
case("edge L/256 = 4097", 1, 8, 4097 * 256, 128, FALLBACK, prescaled=True, strides=strided())
case("edge H = 4096", 1, 4096, 512, 128, GEN + (True,), prescaled=True, strides=(4096 * 128,) * 9, grids=(256, 8192, 0))
case("edge H = 4104", 1, 4104, 512, 128, FALLBACK, prescaled=True, strides=(4104 * 128,) * 9)
# the CU plan: whole XCD rows of 8, only when it leaves fewer CUs than the device has
for plan_cus, g in ((0, G24), (7, G24), (8, (8, 24, 0)), (16, (16, 16, 1)), (20, (16, 16, 1)), (256, G24), (264, G24)):
    case(f"edge plan_cus {plan_cus}", 1, 8, 768, 128, GEN + (True,), prescaled=True, strides=strided(), plan_cus=plan_cus, grids=g)
case("edge dev_cus 64 plan 72", 8, 16, 1280, 128, GEN + (True,), prescaled=True, strides=(16 * 128,) * 9, dev_cus=64, plan_cus=72, grids=(64, 640, 0))
case("edge dev_cus 128", 8, 16, 1280, 128, GEN + (True,), prescaled=True, strides=(16 * 128,) * 9, dev_cus=128, grids=(128, 640, 0))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """build the printer with the host compiler, run it once over the whole table: {case name: {field: value}}"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("attention_plan") / "attention_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "attention_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    names = [n for n, _, _ in CASES]
    assert len(set(names)) == len(names)
    run = subprocess.run([exe], input="".join(f"{line} {name}\n" for name, line, _ in CASES), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {}
    for row in run.stdout.splitlines():
        name, *fields = row.split()
        out[name] = dict(f.split("=") for f in fields)
    assert list(out) == names, "the printer did not answer every case"
    return out


@pytest.mark.parametrize("name,expected", [(n, e) for n, _, e in CASES], ids=[n for n, _, _ in CASES])
def test_plan(plans, name, expected):
    (fwd, dq, dkv, planes), grids = expected
    got = plans[name]
    assert (got["fwd"], got["dq"], got["dkv"], got["planes"]) == (fwd, dq, dkv, str(int(planes))), got
    # a grid is printed for a generated program and for nothing else, and every generated program of the table has its numbers stated
    want = {k for k, prog in (("fwd_grid", fwd), ("dq_grid", dq), ("dkv_grid", dkv)) if prog.endswith("GEN64")}
    assert {k for k in got if k.endswith("_grid")} == want == set(grids), (got, grids)
    for k, g in grids.items():
        assert tuple(int(x) for x in got[k].split("/"))[:len(g)] == tuple(g), (k, got[k], g)
