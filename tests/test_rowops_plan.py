"""Which row kernel runs, on what grid: unidisc_amd/csrc/rowops_plan.h, compiled alone with a host compiler (tests/rowops_plan_print.cpp) and asked for the plan of
every (entry point, M, d, L, flags) that the GPU tests run - tests/test_gpu_rowops_rowwise.py, tests/test_gpu_rowops_d256.py, the row-kernel tests of
tests/test_gpu_kernels.py, and the calls unidisc_amd/dit.py makes on all rows of a batch in every config of tests/test_gpu_fullwidth_oracle.py (the last block's calls on
the [MASK] rows alone have a row count the data decides and are not listed) - so
that a test which believes it exercises one kernel fails HERE when a cap moves it onto another; and of one case on each side of every gate.  The expected plans are
written out below from the launch code this header replaced, not computed from the header.

Workspace offered (`ws`): a number of floats, or ASK: what unidisc_amd.kernels.ROWOPS_WS asks of `_scratch` for the call (the wrappers' path; `_scratch` may hand
over more, which changes no plan: see test_asks_cover_the_plan).  The wrappers offer one to residual_bwd only with a sandwich norm and to qknorm_rope_bwd only with
the four affine gradients in one allocation; the table passes 0 otherwise.

Every instantiation the dispatcher lists of rowops.hip hold - read from its source - is selected by a plan of the table, and no other (test_every_instance_has_a_case).  Three of them are reached by no GPU test:
norm_residual_bwd_wrow_kernel<4> and the NIT = 3, 4 instances of the narrow qk kernels (no GPU width lies in 1536 < d < 2048 or has d % 16 == 0 in 1024 < d < 2048)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASK = "ask"
W, B_, B2 = "WAVE_ROW", "BLOCK_ROW", "BLOCK_ROW_2ROWS"
NOT_OK = None
PLANES = dict(norm_bwd=1, residual_bwd=1, norm_residual_bwd=3, norm_residual_bwd_ada=6, qk_bwd=1)
WS_KEY = dict(norm_bwd="norm_bwd", residual_bwd="residual_bwd", norm_residual_bwd="norm_residual_bwd", norm_residual_bwd_ada="norm_residual_bwd_ada", qk_bwd="qknorm_rope_bwd")

CASES = {}   # name -> (entry, M, d, L, a, b, ws, expected)
ASK_TOO_SMALL = set()   # cases for which the wrapper's ask does not cover a workspace launch (test_asks_cover_the_plan)


def case(entry, M, d, expect, *, L=1, a=0, b=0, ws=0, tag=""):
    """expect = (form, inst, grid[, bpb[, use_ws[, lds_bytes]]]) or NOT_OK.  a, b: the entry point's flags (tests/rowops_plan_print.cpp).  The same call may be
    listed by several tests: it must then be listed with the same expectation."""
    name = f"{entry}:M{M}:d{d}:L{L}:{a}{b}:ws{ws}{tag}"
    if expect is not NOT_OK:
        expect = tuple(expect) + (0, False, 0)[len(expect) - 3:]
    assert CASES.setdefault(name, (entry, M, d, L, a, b, ws, expect))[7] == expect, name


def fwd(M, d, inst, grid):
    case("fwd", M, d, (W, inst, grid))


NCH = {64: 1, 256: 1, 520: 2, 768: 2, 1032: 3, 2048: 4, 3072: 8, 4096: 8}   # chunks of 512 columns; 8 above 2048
WIDTHS = (64, 520, 768, 1032, 2048, 3072, 4096)                          # rowops_ref64.WIDTHS

# ---- tests/test_gpu_rowops_rowwise.py: B, L = 5, 37 on every width (the *_families tests), M = 185 rows in 47 blocks of 4
for d in WIDTHS:
    fwd(185, d, NCH[d], 47)
    case("norm_bwd", 185, d, (W, NCH[d], 47), L=37)                       # M < 2048: the wrapper offers no workspace
    case("norm_bwd", 185, d, (W, NCH[d], 45, 9), L=37, a=1)               # modulated: 47 / 5 = 9 blocks per batch element
    for sandwich, ws in ((0, 0), (1, ASK)):
        if d < 2048:
            case("residual_bwd", 185, d, (W, NCH[d], 47), L=37, b=sandwich, ws=ws)       # grid_rows(M) < 1024: atomics also with a workspace
        elif d == 2048:
            case("residual_bwd", 185, d, (W, 4, 1024, 0, bool(sandwich)), L=37, b=sandwich, ws=ws)
        else:
            case("residual_bwd", 185, d, (B_, 2, 185, 0, bool(sandwich)), L=37, b=sandwich, ws=ws)
        case("residual_bwd", 185, d, (W, NCH[d], 50, 10), L=37, a=1, b=sandwich, ws=ws)   # gated: min(1024 / 5, ceil(37 / 4)) = 10; 50 blocks < 64: atomics
for d, inst in ((64, 1), (520, 2), (768, 2), (1032, 3)):
    case("norm_residual_bwd", 185, d, (W, inst, 47, 0, True), ws=ASK)
for d, inst in ((2048, 1), (4096, 2)):
    case("norm_residual_bwd", 185, d, (B_, inst, 185, 0, True), ws=ASK)
    case("norm_residual_bwd_ada", 185, d, (B_, inst, 185, 37, True), L=37, ws=ASK)        # min(768 / 5, 37) = 37: one block per row
case("norm_residual_bwd", 185, 3072, NOT_OK, ws=ASK)                      # (the wrapper runs norm_bwd and residual_bwd there)
# qk: QK_WIDTHS = 64, 768, 2048, 3072, 4096 (520 and 1032 are no multiple of 16); qk-norm on with one allocation / four tensors, and off
for d, nit in ((64, 1), (768, 2)):
    for qk in (1, 0):
        case("qk_fwd", 185, d, (W, nit, 47, 0, False, 16 * d * qk), a=qk)
        case("qk_bwd", 185, d, (W, nit, 47, 0, False, (8 * d + 16384) * qk), a=qk)
    case("qk_bwd", 185, d, (W, nit, 47, 0, False, 8 * d + 16384), a=1, b=1, ws=ASK)       # 47 blocks < 64: atomics
for qk in (1, 0):
    case("qk_fwd", 185, 2048, (B2, 2, 93), a=qk)                          # 93 groups of two rows, no LDS
    for d in (3072, 4096):
        case("qk_fwd", 185, d, (B_, 2, 185, 0, False, 16 * d * qk), a=qk)
    for d, inst in ((2048, 1), (3072, 2), (4096, 2)):
        case("qk_bwd", 185, d, (B_, inst, 185, 0, False, 8 * d * qk), a=qk)
for d, inst in ((2048, 1), (3072, 2), (4096, 2)):
    case("qk_bwd", 185, d, (B_, inst, 185, 0, True, 8 * d), a=1, b=1, ws=ASK)
# NORM_ROWS
for M, d, g in ((1, 64, 1), (3, 768, 1), (37, 2048, 10), (1, 4096, 1), (1400, 768, 350), (1400, 2048, 350), (2048, 768, 512), (8200, 64, 2048), (2051, 2048, 513), (2050, 4096, 513)):
    fwd(M, d, NCH[d], g)
case("norm_bwd", 1, 64, (W, 1, 1, 1), L=1, a=1)
case("norm_bwd", 3, 768, (W, 2, 1), L=3)
case("norm_bwd", 37, 2048, (W, 4, 10, 10), L=37, a=1)
case("norm_bwd", 1, 4096, (W, 8, 1), L=1)
case("norm_bwd", 1400, 768, (W, 2, 350, 175), L=700, a=1)                 # more rows than blocks; M < 2048: no workspace
case("norm_bwd", 1400, 2048, (W, 4, 350, 175), L=700, a=1)
case("norm_bwd", 2048, 768, (W, 2, 512, 0, True), L=2048, ws=ASK)         # the first M with a workspace
case("norm_bwd", 8200, 64, (W, 1, 1024, 0, True), L=8200, ws=ASK)         # past the 1024-block cap
case("norm_bwd", 8200, 64, (W, 1, 1024, 512, True), L=4100, a=1, ws=ASK)  # modulated with a workspace: 2 x 512
case("norm_bwd", 2051, 2048, (W, 4, 512, 0, True), L=2051, ws=ASK)        # past the 512-block cap of the wide rows
case("norm_bwd", 2050, 4096, (W, 8, 512, 512, True), L=2050, a=1, ws=ASK)
# RESID_ROWS
for M, d, g in ((1, 3072, 1), (3, 2048, 1), (37, 4096, 10), (1400, 4096, 350), (4093, 768, 1024)):
    fwd(M, d, NCH[d], g)
case("residual_bwd", 1, 64, (W, 1, 1), L=1, b=1, ws=ASK)
case("residual_bwd", 3, 2048, (W, 4, 1, 1), L=3, a=1, b=1, ws=ASK)
case("residual_bwd", 37, 4096, (B_, 2, 37, 0, True), L=37, b=1, ws=ASK)
case("residual_bwd", 1, 3072, (W, 8, 1, 1), L=1, a=1)
case("residual_bwd", 1400, 768, (W, 2, 350, 175, True), L=700, a=1, b=1, ws=ASK)          # gated, 350 blocks >= 64: the workspace for dw_b
case("residual_bwd", 1400, 2048, (W, 4, 350, 175), L=700, a=1)
case("residual_bwd", 1400, 4096, (W, 8, 350, 175, True), L=700, a=1, b=1, ws=ASK)
case("residual_bwd", 8200, 64, (W, 1, 512), L=8200)                       # past the 512-block cap
case("residual_bwd", 8200, 64, (W, 1, 1024, 0, True), L=8200, b=1, ws=ASK)
case("residual_bwd", 4093, 768, (W, 2, 1024, 0, True), L=4093, b=1, ws=ASK)               # the wide-grid workspace form: grid_rows(M) = 1024
case("residual_bwd", 2051, 2048, (W, 4, 1024, 0, True), L=2051, b=1, ws=ASK)              # the wave-per-row form of d = 2048
case("residual_bwd", 2051, 2048, (W, 4, 1024), L=2051)
case("residual_bwd", 2050, 4096, (B_, 2, 1536, 0, True), L=2050, b=1, ws=ASK)             # past the 1536-block cap
# FUSED_ROWS
fwd(4100, 64, 1, 1025)
fwd(37, 768, 2, 10)
for d in (2048, 4096):
    fwd(1000, d, NCH[d], 250)
case("norm_residual_bwd", 1, 64, (W, 1, 1, 0, True), ws=ASK)
case("norm_residual_bwd", 3, 2048, (B_, 1, 3, 0, True), ws=ASK)
case("norm_residual_bwd", 37, 768, (W, 2, 10, 0, True), ws=ASK)
case("norm_residual_bwd", 4100, 64, (W, 1, 1024, 0, True), ws=ASK)        # past the 1024-block cap of the wave-per-row form
case("norm_residual_bwd", 1000, 2048, (B_, 1, 768, 0, True), ws=ASK)      # past the 768 blocks of the block-per-row form
case("norm_residual_bwd", 1000, 4096, (B_, 2, 768, 0, True), ws=ASK)
case("norm_residual_bwd_ada", 1, 2048, (B_, 1, 1, 1, True), L=1, ws=ASK)
case("norm_residual_bwd_ada", 1400, 2048, (B_, 1, 768, 384, True), L=700, ws=ASK)         # more rows than blocks
case("norm_residual_bwd_ada", 1400, 4096, (B_, 2, 768, 384, True), L=700, ws=ASK)
# QK_ROWS
case("qk_fwd", 1, 64, (W, 1, 1, 0, False, 1024), a=1)
case("qk_bwd", 1, 64, (W, 1, 1, 0, False, 16896), a=1, b=1, ws=ASK)
case("qk_fwd", 3, 2048, (B2, 2, 2), a=1)                                  # the ragged two-row group
case("qk_bwd", 3, 2048, (B_, 1, 3, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_fwd", 37, 2048, (B2, 2, 19), a=1)
case("qk_bwd", 37, 2048, (B_, 1, 37, 0, False, 16384), a=1)
case("qk_fwd", 1, 4096, (B_, 2, 1, 0, False, 65536), a=1)
case("qk_bwd", 1, 4096, (B_, 2, 1, 0, True, 32768), a=1, b=1, ws=ASK)
case("qk_fwd", 1400, 768, (W, 2, 350, 0, False, 12288), a=1)
case("qk_bwd", 1400, 768, (W, 2, 350, 0, True, 22528), a=1, b=1, ws=ASK)  # the workspace form of the narrow rows (M >= 253)
case("qk_bwd", 1400, 768, (W, 2, 256, 0, False, 22528), a=1)              # four tensors: the 256-block cap of the atomics form
case("qk_fwd", 1400, 2048, (B2, 2, 700), a=1)
case("qk_bwd", 1400, 2048, (B_, 1, 1024, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_bwd", 1400, 2048, (B_, 1, 256, 0, False, 16384), a=1)
case("qk_fwd", 1400, 4096, (B_, 2, 1400, 0, False, 65536), a=1)
case("qk_bwd", 1400, 4096, (B_, 2, 1024, 0, True, 32768), a=1, b=1, ws=ASK)
case("qk_fwd", 4100, 64, (W, 1, 1024, 0, False, 1024), a=1)              # past the 1024-block cap of the narrow forward
case("qk_bwd", 4100, 64, (W, 1, 1024, 0, True, 16896), a=1, b=1, ws=ASK)
case("qk_bwd", 4100, 64, (W, 1, 256, 0, False, 16896), a=1)
case("qk_fwd", 2051, 2048, (B2, 2, 1024), a=1)                            # 1026 groups, the last one ragged
case("qk_bwd", 2051, 2048, (B_, 1, 1024, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_fwd", 2050, 4096, (B_, 2, 2048, 0, False, 65536), a=1)          # past the 2048-block cap
case("qk_bwd", 2050, 4096, (B_, 2, 1024, 0, True, 32768), a=1, b=1, ws=ASK)
case("qk_bwd", 2050, 4096, (B_, 2, 256, 0, False, 32768), a=1)
# test_wider_than_4096_is_refused (M = 8, d = 4104) - and the same width at every other entry point
case("fwd", 8, 4104, NOT_OK)
case("norm_bwd", 8, 4104, NOT_OK, L=8)
case("norm_bwd", 8, 4104, NOT_OK, L=8, a=1)
case("residual_bwd", 8, 4104, NOT_OK, L=8, b=1, ws=ASK)
case("residual_bwd", 8, 4104, NOT_OK, L=8, a=1)
case("norm_residual_bwd", 8, 4104, NOT_OK, ws=ASK)
case("norm_residual_bwd_ada", 8, 4104, NOT_OK, L=8, ws=ASK)
case("qk_fwd", 8, 4104, NOT_OK, a=1)
case("qk_bwd", 8, 4104, NOT_OK, a=1, b=1, ws=ASK)

# ---- tests/test_gpu_rowops_d256.py (M = 40; d = 512, 4096) and test_qknorm_rope of tests/test_gpu_kernels.py (M = 40; d = 64, 768, 2048, 256).  The four gradients are
# four allocations, which the allocator may or may not place back to back: both forms
for d, nit in ((64, 1), (256, 1), (512, 1), (768, 2)):
    for qk in (1, 0):
        case("qk_fwd", 40, d, (W, nit, 10, 0, False, 16 * d * qk), a=qk)
        case("qk_bwd", 40, d, (W, nit, 10, 0, False, (8 * d + 16384) * qk), a=qk)
    case("qk_bwd", 40, d, (W, nit, 10, 0, False, 8 * d + 16384), a=1, b=1, ws=ASK)
for qk in (1, 0):
    case("qk_fwd", 40, 2048, (B2, 2, 20), a=qk)
    case("qk_fwd", 40, 4096, (B_, 2, 40, 0, False, 65536 * qk), a=qk)
    case("qk_bwd", 40, 2048, (B_, 1, 40, 0, False, 16384 * qk), a=qk)
    case("qk_bwd", 40, 4096, (B_, 2, 40, 0, False, 32768 * qk), a=qk)
case("qk_bwd", 40, 2048, (B_, 1, 40, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_bwd", 40, 4096, (B_, 2, 40, 0, True, 32768), a=1, b=1, ws=ASK)

# ---- the norm / residual tests of tests/test_gpu_kernels.py: d = 64, 768, 2048 at B, L = 3, 37 / 3, 40 / 2, 24 / 5, 37 (above); M = 1000 at 2048, 4096, 768, 256, 1032
for d in (64, 768, 2048):
    fwd(111, d, NCH[d], 28)
    fwd(120, d, NCH[d], 30)
    fwd(48, d, NCH[d], 12)
    case("norm_bwd", 120, d, (W, NCH[d], 30), L=40)
    case("norm_bwd", 120, d, (W, NCH[d], 30, 10), L=40, a=1)
    for sandwich, ws in ((0, 0), (1, ASK)):
        case("residual_bwd", 48, d, (W, NCH[d], 12) if d < 2048 else (W, 4, 1024, 0, bool(sandwich)), L=24, b=sandwich, ws=ws)
        case("residual_bwd", 48, d, (W, NCH[d], 12, 6), L=24, a=1, b=sandwich, ws=ws)
fwd(1400, 2048, 4, 350)
case("norm_bwd", 111, 2048, (W, 4, 28), L=37)
case("norm_bwd", 111, 2048, (W, 4, 27, 9), L=37, a=1)
case("norm_bwd", 1400, 2048, (W, 4, 350), L=700)
for sandwich, ws in ((0, 0), (1, ASK)):   # test_norm_residual_bwd_ada_equals_separate_kernels: d = 2048
    case("residual_bwd", 111, 2048, (W, 4, 30, 10), L=37, a=1, b=sandwich, ws=ws)
    case("residual_bwd", 111, 2048, (W, 4, 1024, 0, bool(sandwich)), L=37, b=sandwich, ws=ws)
    case("residual_bwd", 1400, 2048, (W, 4, 350, 175, bool(sandwich)), L=700, a=1, b=sandwich, ws=ws)
    case("residual_bwd", 1400, 2048, (W, 4, 1024, 0, bool(sandwich)), L=700, b=sandwich, ws=ws)
case("norm_residual_bwd_ada", 111, 2048, (B_, 1, 111, 37, True), L=37, ws=ASK)
for d in (256, 768, 1032, 2048, 4096):    # test_norm_residual_bwd_fused_equals_the_two_kernels: M = 1000
    fwd(1000, d, NCH[d], 250)
    case("norm_bwd", 1000, d, (W, NCH[d], 250), L=250)
    for sandwich, ws in ((0, 0), (1, ASK)):
        expect = (W, NCH[d], 250) if d < 2048 else ((W, 4, 1024, 0, bool(sandwich)) if d == 2048 else (B_, 2, 1000, 0, bool(sandwich)))
        case("residual_bwd", 1000, d, expect, L=250, b=sandwich, ws=ws)
    case("norm_residual_bwd", 1000, d, (W, NCH[d], 250, 0, True) if d < 2048 else (B_, 1 if d == 2048 else 2, 768, 0, True), ws=ASK)
fwd(64, 256, 1, 16)                       # the dropout mask tests
fwd(1024, 2048, 4, 256)
case("residual_bwd", 64, 256, (W, 1, 16), L=32)

# ---- tests/test_gpu_fullwidth_oracle.py: the calls unidisc_amd/dit.py makes on all M = B L rows, config by config.  Without adaLN the last block works behind its
# attention on the [MASK] rows only, a number of rows the data decides (not listed) - unless the padded count reaches M, when it runs on all rows like the blocks
# below it.  The four qk-norm gradients are slices of the flat gradient buffer: both layouts are listed.
def engine_forward(M, d, nch, grid, qk_fwd_plan, qk):
    """block 0's norm1 (norm_fwd), every block's two residual adds with the next pre-norm fused (residual_norm_fwd[_ada]): one plan; qknorm_rope_fwd"""
    fwd(M, d, nch, grid)
    case("qk_fwd", M, d, qk_fwd_plan, a=qk)


# _LARGE (d = 2048, rms, qk-norm, sandwich norms), L = 1280: config_c_1block_b8, _2blocks_b2, _24blocks_b2 (M = 10240, 2560, 2560); the forward-only test (B = 2);
# _PACKED, L = 4608: config_e_1block_b2 (M = 9216)
for M, L, g in ((10240, 1280, 2048), (2560, 1280, 640), (9216, 4608, 2048)):
    engine_forward(M, 2048, 4, g, (B2, 2, 1024), 1)
    # backward, top down: [final norm + last block's MLP branch, its norm2 + attention branch: fused passes on the rows that block ran on]; qknorm_rope_bwd; every
    # norm1 with the MLP branch of the block below, every norm2 with its attention branch: norm_residual_bwd; block 0's norm1 alone: norm_bwd
    case("norm_residual_bwd", M, 2048, (B_, 1, 768, 0, True), ws=ASK)
    case("qk_bwd", M, 2048, (B_, 1, 1024, 0, True, 16384), a=1, b=1, ws=ASK)
    case("qk_bwd", M, 2048, (B_, 1, 256, 0, False, 16384), a=1)
    case("norm_bwd", M, 2048, (W, 4, 512, 0, True), L=L, ws=ASK)
# the same with adaLN (config_c_adaln_1block_b8, _2blocks_b2): no compaction, every call on all rows.  Backward: the final norm modulated (norm_bwd); the last
# block's MLP branch gated behind its sandwich norm (residual_bwd); every other pair as norm_residual_bwd_ada; block 0's modulated norm1 alone (norm_bwd)
for M, B, bpb_n, g_r, bpb_r in ((10240, 8, 64, 1024, 128), (2560, 2, 256, 640, 320)):
    case("norm_bwd", M, 2048, (W, 4, 512, bpb_n, True), L=1280, a=1, ws=ASK)             # min(512 / B, 320 blocks of 4 rows)
    case("residual_bwd", M, 2048, (W, 4, g_r, bpb_r, True), L=1280, a=1, b=1, ws=ASK)     # min(1024 / B, 320)
    case("norm_residual_bwd_ada", M, 2048, (B_, 1, 768, 768 // B, True), L=1280, ws=ASK)
# _SMALL (d = 768, rms, qk-norm, sandwich norms): unidisc_s_12blocks_b4, M = 4 x 384
engine_forward(1536, 768, 2, 384, (W, 2, 384, 0, False, 12288), 1)
case("norm_residual_bwd", 1536, 768, (W, 2, 384, 0, True), ws=ASK)
case("qk_bwd", 1536, 768, (W, 2, 384, 0, True, 22528), a=1, b=1, ws=ASK)
case("qk_bwd", 1536, 768, (W, 2, 256, 0, False, 22528), a=1)
case("norm_bwd", 1536, 768, (W, 2, 384), L=384)                           # M < 2048: atomics
# _PLUMB (d = 256, LayerNorm, no qk-norm, no sandwich norm), L = 128.  config_a_plumbing_b8 (adaLN, M = 1024; the fused adaLN form is built for d = 2048 / 4096
# only): every norm backward modulated, both residual branches gated, each its own launch
engine_forward(1024, 256, 1, 256, (W, 1, 256), 0)
case("norm_bwd", 1024, 256, (W, 1, 256, 32), L=128, a=1)
case("residual_bwd", 1024, 256, (W, 1, 256, 32), L=128, a=1)
case("qk_bwd", 1024, 256, (W, 1, 256), a=0)
# layernorm_no_adaln_b4 (M = 512): the schedule of the models without adaLN
engine_forward(512, 256, 1, 128, (W, 1, 128), 0)
case("norm_residual_bwd", 512, 256, (W, 1, 128, 0, True), ws=ASK)
case("qk_bwd", 512, 256, (W, 1, 128), a=0)
case("norm_bwd", 512, 256, (W, 1, 128), L=128)

# ---- one case on each side of every gate
# grid_rows: 2048 blocks of 4 rows; the instance by width
fwd(8188, 64, 1, 2047)
fwd(8192, 64, 1, 2048)
fwd(8193, 64, 1, 2048)
for d, inst in ((512, 1), (1024, 2), (1536, 3), (1544, 4), (2056, 8)):
    fwd(8, d, inst, 2)
# norm_bwd: the cap by width, the 64-block gate of the workspace, a workspace too small, no workspace
case("norm_bwd", 8200, 2040, (W, 4, 1024, 0, True), L=8200, ws=ASK)
case("norm_bwd", 8200, 2048, (W, 4, 512, 0, True), L=8200, ws=ASK)
case("norm_bwd", 2047, 768, (W, 2, 512, 0, True), L=2047, ws=1024 * 768)  # the M >= 2048 gate is the wrapper's, not the plan's
case("norm_bwd", 2047, 768, (W, 2, 512), L=2047, ws=ASK)
case("norm_bwd", 256, 768, (W, 2, 64, 0, True), L=256, ws=1024 * 768)
case("norm_bwd", 252, 768, (W, 2, 63), L=252, ws=1024 * 768)
case("norm_bwd", 2048, 768, (W, 2, 512, 0, True), L=2048, ws=512 * 768)
case("norm_bwd", 2048, 768, (W, 2, 512), L=2048, ws=512 * 768 - 1)
case("norm_bwd", 8200, 64, (W, 1, 512), L=8200)                           # without a workspace the unmodulated grid is capped at 512 ...
case("norm_bwd", 8200, 64, (W, 1, 1024, 512), L=4100, a=1)                # ... the modulated one is not
case("norm_bwd", 1600, 64, (W, 1, 800, 1), L=2, a=1)                     # more batch elements (800) than blocks (400): one block each
# a modulated call of more than 1024 batch elements: one block each, 2050 partial rows - more than the 1024 the wrapper asks for at any M >= 2048, so through the
# wrapper this shape stays on atomics although the plan would take a workspace (no preset has such a batch; see test_asks_cover_the_plan)
case("norm_bwd", 4100, 64, (W, 1, 2050, 1), L=2, a=1, ws=ASK)
ASK_TOO_SMALL.add("norm_bwd:M4100:d64:L2:10:wsask")
# residual_bwd, gated: the 64-block gate, a workspace too small
case("residual_bwd", 256, 768, (W, 2, 64, 32, True), L=128, a=1, b=1, ws=ASK)
case("residual_bwd", 248, 768, (W, 2, 62, 31), L=124, a=1, b=1, ws=ASK)
case("residual_bwd", 1400, 768, (W, 2, 350, 175), L=700, a=1, b=1, ws=350 * 768 - 1)
# ungated: d = 2048 without room for 1024 partial rows takes the block-per-row form <1>, with or without its own workspace; the widths around 2048; the caps
case("residual_bwd", 2051, 2048, (B_, 1, 256), L=2051, b=1, ws=1024 * 2048 - 1)
case("residual_bwd", 100, 2048, (B_, 1, 100, 0, True), L=100, b=1, ws=100 * 2048)
case("residual_bwd", 100, 2048, (B_, 1, 100), L=100, b=1, ws=100 * 2048 - 1)
case("residual_bwd", 2051, 2040, (W, 4, 512), L=2051)
case("residual_bwd", 2051, 2056, (B_, 2, 1536), L=2051)
case("residual_bwd", 1536, 4096, (B_, 2, 1536, 0, True), L=1536, b=1, ws=ASK)
case("residual_bwd", 1537, 4096, (B_, 2, 1536, 0, True), L=1537, b=1, ws=ASK)
case("residual_bwd", 2050, 4096, (B_, 2, 256), L=2050, b=1, ws=1536 * 4096 - 1)
case("residual_bwd", 2050, 4096, (B_, 2, 256), L=2050, b=1)
case("residual_bwd", 4092, 768, (W, 2, 512), L=4092, b=1, ws=ASK)         # grid_rows(M) = 1023
case("residual_bwd", 4093, 768, (W, 2, 1024, 0, True), L=4093, b=1, ws=1024 * 768)
case("residual_bwd", 4093, 768, (W, 2, 512), L=4093, b=1, ws=1024 * 768 - 1)
case("residual_bwd", 4093, 768, (W, 2, 512), L=4093, ws=1024 * 768)       # no sandwich norm: nothing to sum
# the fused forms: the widths, the caps
case("norm_residual_bwd", 8, 56, NOT_OK, ws=ASK)
case("norm_residual_bwd", 8, 2040, (W, 4, 2, 0, True), ws=ASK)
case("norm_residual_bwd", 8, 2056, NOT_OK, ws=ASK)
case("norm_residual_bwd", 4092, 64, (W, 1, 1023, 0, True), ws=ASK)
case("norm_residual_bwd", 4096, 64, (W, 1, 1024, 0, True), ws=ASK)
case("norm_residual_bwd", 767, 2048, (B_, 1, 767, 0, True), ws=ASK)
case("norm_residual_bwd", 768, 2048, (B_, 1, 768, 0, True), ws=ASK)
case("norm_residual_bwd_ada", 8, 3072, NOT_OK, L=8, ws=ASK)
case("norm_residual_bwd_ada", 9, 2048, NOT_OK, L=2, ws=ASK)               # M is no multiple of L
case("norm_residual_bwd_ada", 1536, 2048, (B_, 1, 768, 1, True), L=2, ws=ASK)
case("norm_residual_bwd_ada", 769, 2048, (B_, 1, 769, 1, True), L=1, ws=ASK, tag=":wrapper_refuses")   # (kernels.norm_residual_bwd_ada_ok: B <= 768)
# qk forward: NIT by width, the three forms around 2048, the caps
for d, nit in ((512, 1), (528, 2), (1024, 2), (1040, 3), (1536, 3), (1552, 4), (2032, 4)):
    case("qk_fwd", 8, d, (W, nit, 2, 0, False, 16 * d), a=1)
    case("qk_bwd", 8, d, (W, nit, 2, 0, False, 8 * d + 16384), a=1)
case("qk_fwd", 8, 2064, (B_, 2, 8, 0, False, 16 * 2064), a=1)
case("qk_fwd", 8, 4112, NOT_OK, a=1)
case("qk_bwd", 8, 4112, NOT_OK, a=1)
case("qk_fwd", 4092, 64, (W, 1, 1023, 0, False, 1024), a=1)
case("qk_fwd", 4096, 64, (W, 1, 1024, 0, False, 1024), a=1)
case("qk_fwd", 2046, 2048, (B2, 2, 1023), a=1)
case("qk_fwd", 2047, 2048, (B2, 2, 1024), a=1)
case("qk_fwd", 2047, 4096, (B_, 2, 2047, 0, False, 65536), a=1)
case("qk_fwd", 2048, 4096, (B_, 2, 2048, 0, False, 65536), a=1)
# qk backward, narrow: the 64-block gate, a workspace too small, four tensors with a workspace, the caps; wide: the same
case("qk_bwd", 253, 768, (W, 2, 64, 0, True, 22528), a=1, b=1, ws=ASK)
case("qk_bwd", 252, 768, (W, 2, 63, 0, False, 22528), a=1, b=1, ws=ASK)
case("qk_bwd", 1400, 768, (W, 2, 256, 0, False, 22528), a=1, b=1, ws=350 * 4 * 768 - 1)
case("qk_bwd", 1400, 768, (W, 2, 256, 0, False, 22528), a=1, b=0, ws=4096 * 768)
case("qk_bwd", 1020, 768, (W, 2, 255, 0, False, 22528), a=1)
case("qk_bwd", 4092, 64, (W, 1, 1023, 0, True, 16896), a=1, b=1, ws=ASK)
case("qk_bwd", 1023, 2048, (B_, 1, 1023, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_bwd", 1025, 2048, (B_, 1, 1024, 0, True, 16384), a=1, b=1, ws=ASK)
case("qk_bwd", 1025, 2048, (B_, 1, 256, 0, False, 16384), a=1, b=1, ws=4096 * 2048 - 1)
case("qk_bwd", 255, 2048, (B_, 1, 255, 0, False, 16384), a=1)
case("qk_bwd", 2050, 4096, (B_, 2, 1024), a=0)                            # rotation only: no sums, no 256-block cap
case("qk_bwd", 8, 2064, (B_, 2, 8, 0, False, 8 * 2064), a=1)

# the kernel template(s) behind a plan, by (entry, the flag that is a template argument there: modulated / gated / adaLN, form) -> (kernel, that flag)
KERNELS = {("fwd", 0, W): [("norm_fwd_kernel", 0), ("residual_fwd_kernel", 0)],
           ("norm_bwd", 0, W): [("norm_bwd_kernel", 0)], ("norm_bwd", 1, W): [("norm_bwd_kernel", 1)],
           ("residual_bwd", 0, W): [("residual_bwd_kernel", 0)], ("residual_bwd", 1, W): [("residual_bwd_kernel", 1)], ("residual_bwd", 0, B_): [("residual_bwd_brow_kernel", 0)],
           ("norm_residual_bwd", 0, W): [("norm_residual_bwd_wrow_kernel", 0)], ("norm_residual_bwd", 0, B_): [("norm_residual_bwd_kernel", 0)],
           ("norm_residual_bwd_ada", 0, B_): [("norm_residual_bwd_kernel", 1)],
           ("qk_fwd", 0, W): [("qknorm_rope_fwd_kernel", 0)], ("qk_fwd", 0, B_): [("qknorm_rope_fwd_brow_kernel", 0)], ("qk_fwd", 0, B2): [("qknorm_rope_fwd_brow_rows_kernel", 0)],
           ("qk_bwd", 0, W): [("qknorm_rope_bwd_kernel", 0)], ("qk_bwd", 0, B_): [("qknorm_rope_bwd_brow_kernel", 0)]}
HUGE = 1 << 40


def _ask(K, entry, M, d, a, b):
    """what the wrapper of unidisc_amd/kernels.py offers for this call"""
    if entry not in WS_KEY or (entry == "residual_bwd" and not b) or (entry == "qk_bwd" and not (a and b)):
        return 0
    return K.ROWOPS_WS[WS_KEY[entry]](M, d)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """build the printer with the host compiler, run it once over the whole table - every case with the workspace it states, with the wrapper's ask and with more
    than any launch needs: {case name: {"": plan, "ask": plan, "huge": plan}}, a plan being {field: value}"""
    from unidisc_amd import kernels as K
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("rowops_plan") / "rowops_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "rowops_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    lines = []
    for name, (entry, M, d, L, a, b, ws, _) in CASES.items():
        ask = _ask(K, entry, M, d, a, b)
        for kind, offered in (("", ask if ws == ASK else ws), ("ask", ask), ("huge", HUGE)):
            lines.append(f"{entry} {M} {d} {L} {a} {b} {offered} {name}|{kind}\n")
    run = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {}
    for row in run.stdout.splitlines():
        key, *fields = row.split()
        name, kind = key.split("|")
        out.setdefault(name, {})[kind] = dict(f.split("=") for f in fields)
    assert list(out) == list(CASES) and all(len(v) == 3 for v in out.values()), "the printer did not answer every case"
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_plan(plans, name):
    entry, M, d, L, a, b, ws, expect = CASES[name]
    got = plans[name][""]
    if expect is NOT_OK:
        assert got["ok"] == "0", got
        return
    form, inst, grid, bpb, use_ws, lds = expect
    assert got["ok"] == "1", got
    assert (got["form"], int(got["inst"]), int(got["grid"]), int(got["bpb"]), got["ws"], int(got["lds"])) == (form, inst, grid, bpb, str(int(use_ws)), lds), got
    # the reduction reads one partial row per block: d columns, 4 d of the qk backward; the workspace holds 1, 3 or 6 such planes
    cols = 4 * d if entry == "qk_bwd" else d
    assert got["reduce"] == (f"{grid}x{cols}" if use_ws else "0x0"), got
    assert int(got["need"]) == (grid * cols * PLANES[entry] if use_ws else 0), got


def launchable():
    """every row-kernel instantiation the entry points of rowops.hip can launch, read from its source: {(kernel, second template argument given, instance)} from the
    lists of the with_inst<...> calls and from the launches of one fixed instance"""
    src = open(os.path.join(ROOT, "unidisc_amd", "csrc", "rowops.hip")).read()
    src = src[src.index("bool with_inst("):src.index("small_batch_linear_bwd_kernel")]
    out = set()
    for insts, kernel, flag in re.findall(r"with_inst<([0-9, ]+)>\(plan\.inst, \[&\]\(auto n\) \{ launch_rows\((\w+)<decltype\(n\)::value(, true)?>", src):
        out |= {(kernel, int(bool(flag)), int(n)) for n in insts.split(",")}
    out |= {(kernel, 0, int(n)) for kernel, n in re.findall(r"launch_rows\((\w+)<(\d+)>", src)}
    assert src.count("launch_rows(") == 1 + len(re.findall(r"launch_rows\(\w+<", src)) and src.count("with_inst<") == len(re.findall(r"with_inst<[0-9, ]+>\(plan\.inst, \[&\]", src))
    return out


def test_every_instance_has_a_case(plans):
    """The instantiations the plans of the table select are exactly those the dispatcher lists of rowops.hip hold: an instantiation without a case is either dead
    (delete it) or a gap of this table, and a plan that names an instance no list holds would launch nothing."""
    template_flag = dict(norm_bwd=True, residual_bwd=True)   # modulated / gated are template arguments there
    seen = {(e, a if template_flag.get(e) else 0, plans[n][""]["form"], int(plans[n][""]["inst"])) for n, (e, _, _, _, a, *_) in CASES.items() if plans[n][""]["ok"] == "1"}
    selected = {(kernel, flag, inst) for e, a, form, inst in seen for kernel, flag in KERNELS[(e, a, form)]}
    can = launchable()
    assert selected == can, (sorted(selected - can), sorted(can - selected))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[0] in WS_KEY])
def test_asks_cover_the_plan(plans, name):
    """The workspace unidisc_amd/kernels.py asks `_scratch` for (ROWOPS_WS) against the plan chosen when exactly that much is offered: the ask is 0 or covers what the
    launch reads and writes, and it is never the ask that keeps a launch off the workspace - the plan under the ask is the plan under any larger buffer (`_scratch`
    hands over its whole buffer), so a call that stays on atomics does so by the plan's own gates.  The two fused forms have no atomics form: the wrapper's shape
    gates are the plan's, and an ask is always used.  This is asserted for the shapes of the table, not for all: ASK_TOO_SMALL names the listed shape for which it does
    not hold (a modulated norm_bwd of more than 1024 batch elements), and asserts that."""
    from unidisc_amd import kernels as K
    entry, M, d, L, a, b, _, _ = CASES[name]
    at_ask, at_huge = plans[name]["ask"], plans[name]["huge"]
    ask = _ask(K, entry, M, d, a, b)
    if entry == "norm_residual_bwd":
        assert K.norm_residual_bwd_fused_ok(d) == (at_ask["ok"] == "1")
    if entry == "norm_residual_bwd_ada":
        assert not K.norm_residual_bwd_ada_ok(M, d, L) or at_ask["ok"] == "1"
        if not K.norm_residual_bwd_ada_ok(M, d, L):
            return
    if at_ask["ok"] == "0":
        return
    assert ask == 0 or ask >= int(at_ask["need"]), (ask, at_ask)
    if name in ASK_TOO_SMALL:   # the known exception: with a larger buffer the plan would use a workspace of more rows than the ask holds
        assert ask and at_ask["ws"] == "0" and at_huge["ws"] == "1" and int(at_huge["need"]) > ask, (ask, at_ask, at_huge)
        return
    if ask:
        assert at_ask == at_huge, (at_ask, at_huge)
    if entry.startswith("norm_residual_bwd") or (entry == "norm_bwd" and ask and int(at_ask["grid"]) >= 64):
        assert ask > 0 and at_ask["ws"] == "1", (ask, at_ask)
