"""Which GEMM kernel runs, on what grid, in how many K slices: unidisc_amd/csrc/gemm_plan.h, compiled alone with a host compiler (tests/gemm_plan_print.cpp) and asked
for the plan of every call the GPU tests make - the lists of tests/gemm_ref64.py under the switches tests/test_gpu_gemm_exact.py sets for them, its GELU sweep, every GEMM
shape of tests/test_gpu_kernels.py (the gemm_set_cus test at its three caps), the GEMMs unidisc_amd/dit.py issues on all rows of a batch in the configs of
tests/test_gpu_fullwidth_oracle.py (d = 2048 at M = 10240 / 2560 / 9216, d = 768 at M = 1536, d = 256 at M = 1024 / 512), the shapes whose measured choice gemm_plan.h
records - so that a test which believes it exercises one kernel fails HERE when a gate moves it onto another; and of one case on each side of every gate.  The expected
plans are written out below from the launch code this header replaced (udm_gemm_*_bf16 of gemm.hip with choose_tile / persistent_wide_ok, udm_quad_*_ok and launch_quad_t
of gemm_quad.hip), not computed from the header.

The cost model in short (choose_tile): time ~ rounds x tile area / efficiency = rounds x {44281 (128 x 128, 512 slots), 52852 (192), 65536 (256), 81920 (320 rows, 256
slots)}, x 1.15 for K <= 1024 unless the shape is persistent (whole 256- / 320-row tiles, more than 256 of them), x 0.90 where it is; ties go to the larger tile.

Every kernel instantiation the dispatchers of gemm.hip / gemm_quad.hip can launch - read from their source - is selected by a plan of the table, and no other
(test_every_instance_has_a_case).  Reached by no GPU test (the cases tagged `extra` alone select them): the K-major 8-wave kernel on 320-row tiles (TN: no
K-major shape of the GPU tests is one for which the cost model picks 320-row tiles and the quad kernel does not fit; the case here forces the tile), the persistent form of the 8-wave kernel with a bias epilogue and bf16 output,
with GELU' and fp32 output and (256-row tiles only; the 320-row one runs with beta = 1 in test_gemm_persistent_blocks_every_epilogue) with a plain fp32 output, and the
generated asm K loop under the GELU / GELU' epilogue on 320-row tiles (auto mode keeps those epilogues on the 8-wave kernels; gemm_set_quad(2) tests run them on 256-row tiles)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, STAGGER, PERSIST, QUAD, RAGGED = "SMALL", "STAGGER", "PERSIST", "QUAD", "QUAD_RAGGED"
NONE, BIAS, GELU, DGELU = 0, 1, 2, 3
NOT_OK, FALLBACK = "not ok", "fallback"
ASK, HUGE = "ask", 1 << 40
ENV = dict(cus=256, quad=1, persist=1, tile=-1, ragged=1, asm=1)
# (epilogue, out_f32, beta) of the variants of tests/test_gpu_gemm_exact.py
VARIANTS = dict(none_bf16=(NONE, 0, 0), none_f32=(NONE, 1, 0), bias_bf16=(BIAS, 0, 0), bias_f32=(BIAS, 1, 0), gelu=(GELU, 0, 0), dgelu_bf16=(DGELU, 0, 0),
                dgelu_f32=(DGELU, 1, 0), beta1=(NONE, 1, 1))

CASES = {}   # name -> (entry, args, env, expect, extra)
ASK_TOO_SMALL = set()   # cases for which the wrapper's ask does not cover the split the plan would take with a larger buffer (test_asks_cover_the_plan): none


def up(n, m):
    return (n + m - 1) // m * m


def plan(family, rows, grid, *, sk=1, asm=0, finish="none", reduce="none", rgrid=(0, 0), need=0):
    return dict(family=family, rows=rows, grid=grid, splitk=sk, asm=asm, finish=finish, reduce=reduce, rgrid="%d+%d" % rgrid, need=need)


def ws_plan(family, rows, tiles, sk, area, reduce, rgrid2=0, rgrid=None):
    """a workspace split: grid = tiles x slices, need = slices x area floats, the reduce pass over area / 4 float4s in blocks of 256 (at most 2048 blocks)"""
    return plan(family, rows, tiles * sk, sk=sk, finish="ws", reduce=reduce, rgrid=(rgrid if rgrid is not None else min(-(-area // 1024), 2048), rgrid2), need=sk * area)


def case(entry, args, expect, *, extra=False, **env):
    """The same call may be listed by several tests: it must then be listed with the same expectation."""
    e = dict(ENV, **env)
    name = entry + ":" + "x".join(str(a) for a in args) + "".join(f":{k}{v}" for k, v in env.items())
    got = CASES.setdefault(name, (entry, tuple(args), e, expect, extra))
    assert got[3] == expect, name
    if not extra and got[4]:
        CASES[name] = got[:4] + (False,)


def nt(M, N, K, expect, epi=NONE, f32=0, beta=0, *, ldc=None, ldaux=None, **kw):
    ldc = up(N, 8) if ldc is None else ldc
    ldaux = (up(N, 8) if epi >= GELU else 0) if ldaux is None else ldaux
    case("nt", (M, N, K, ldc, ldaux, epi, f32, beta), expect, **kw)


def nt_exact(M, N, K, variant, expect, **kw):
    """as nt_case of tests/test_gpu_gemm_exact.py places the operands: bf16 C / aux with row stride up(N, 8) + 8, fp32 C with up(N, 4) + 4"""
    epi, f32, beta = VARIANTS[variant]
    nt(M, N, K, expect, epi, f32, beta, ldc=up(N, 4) + 4 if f32 else up(N, 8) + 8, ldaux=up(N, 8) + 8 if epi >= GELU else 0, **kw)


def tn(M, N, K, expect, beta=0, **kw):
    case("tn", (M, N, K, beta), expect, **kw)


def splitk(entry, M, N, K, expect, *, ldc=None, ws=ASK, **kw):
    case(entry, (M, N, K, N if ldc is None else ldc, ws), expect, **kw)


def nn(M, N, K, expect, **kw):
    case("nn", (M, N, K), expect, **kw)


def pair(M0, M1, N, K, expect, *, contiguous=1, ws=ASK, **kw):
    case("tn_pair", (M0, M1, N, K, contiguous, ws), expect, **kw)


def multi(shapes, K, expect, *, ws=ASK, **kw):
    case("tn_multi", (K, ws) + tuple(x for s in shapes for x in s), expect, **kw)


# ================================================================================================ tests/gemm_ref64.py under the switches of tests/test_gpu_gemm_exact.py
# NT_SMALL: M < 192, or N < 192, or K % 64 != 0, or K < 128 -> the 128 x 128 kernel on ceil(M / 128) x ceil(N / 128) blocks, whatever the epilogue
for (M, N, K), grid in (((8, 384, 32), 3), ((200, 136, 72), 4), ((136, 1001, 256), 16), ((40, 64, 2056), 1), ((129, 129, 8), 4)):
    for v in VARIANTS:
        nt_exact(M, N, K, v, plan(SMALL, 128, grid))
for v, (epi, f32, beta) in VARIANTS.items():   # test_nt_small_kernel_narrow_ldc: ldc = ldaux = 139 (N + 3)
    if v != "bias_f32":
        nt(200, 136, 72, plan(SMALL, 128, 4), epi, f32, beta, ldc=139, ldaux=139 if epi >= GELU else 0)
# NT_STAGGER under gemm_set_tile: the forced tile (K % 64 == 0, K >= 128), ceil(M / tile) x ceil(N / 256) blocks; ragged M: never persistent
for (M, N, K), grids in (((333, 260, 128), {192: 4, 256: 4, 320: 4, 0: 9}), ((700, 1001, 192), {192: 16, 256: 12, 320: 12, 0: 48})):
    for tile, grid in grids.items():
        for v in VARIANTS:
            nt_exact(M, N, K, v, plan(STAGGER, tile, grid) if tile else plan(SMALL, 128, grid), tile=tile)
# NT_PERSIST (tile 256) / NT_PERSIST_320 (tile 320): 17 x 16 = 272 whole tiles > 256 -> 256 persistent blocks; gemm_set_persist(0): one block per tile
for tile, (M, N, K) in ((256, (4352, 4096, 128)), (256, (4352, 4096, 192)), (320, (5440, 4096, 128))):
    for v in ("none_bf16", "bias_f32", "gelu", "dgelu_bf16"):
        nt_exact(M, N, K, v, plan(PERSIST, tile, 256), tile=tile)
        nt_exact(M, N, K, v, plan(STAGGER, tile, 272), tile=tile, persist=0)
# NT_QUAD under gemm_set_quad(2): one tile row of fm = M / 64, N / 256 blocks.  K = 128, 192, 448 are 2, 3, 7 K tiles: the generated asm K loop needs at least 4 and an
# even count, so asm = 1 selects the C++ loop there as asm = 0 does; K = 256 (4 K tiles, NT_QUAD_ASM) takes it on the 256- and 320-row tiles (fm = 3 has none)
for M in (192, 256, 320):
    for N in (256, 512):
        for K in (128, 192, 448) + ((256,) if M > 192 else ()):
            for asm in (1, 0):
                for v in ("none_bf16", "bias_bf16", "none_f32"):
                    nt_exact(M, N, K, v, plan(QUAD, M, N // 256, asm=1 if (K == 256 and asm) else 0), quad=2, asm=asm)
# NT_QUAD_RAGGED (5000, 2048, 128): choose_tile takes ONE round of 192-row tiles (27 x 8 = 216 tiles: 52852 x 1.15 against 65536 x 1.15 and 81920 x 1.15), no quad tile is
# whole -> the 8-wave kernel.  NT_QUAD_RAGGED_320 (8200, 2048, 128): 192- and 256-row tiles need two rounds (344, 264 tiles), 320-row tiles one (26 x 8 = 208) -> fm = -5
for v in ("none_bf16", "bias_bf16"):
    nt_exact(5000, 2048, 128, v, plan(STAGGER, 192, 216), quad=2)
    nt_exact(8200, 2048, 128, v, plan(RAGGED, 320, 208), quad=2)
# NN: gemm_nn then gemm_nn_splitk (slices at least FOUR K tiles deep; the wrapper offers 32 M N floats up to M N = 2^22)
nn(192, 256, 128, plan(QUAD, 192, 1))
nn(320, 256, 256, plan(QUAD, 320, 1))
nn(768, 256, 1024, plan(QUAD, 192, 4))          # 4 tiles of 192 rows (one round x 192) before 3 of 256
nn(5000, 2048, 128, plan(RAGGED, 320, 128))     # 16 x 8 = 128 ragged tiles, no whole tile height
splitk("nn_splitk", 192, 256, 128, FALLBACK, ldc=264)     # 2 K tiles: no slice of 4
splitk("nn_splitk", 320, 256, 256, FALLBACK, ldc=264)     # 4 K tiles: one slice
splitk("nn_splitk", 768, 256, 1024, ws_plan(QUAD, 192, 4, 4, 768 * 256, "bf16"), ldc=264)   # min(256 / 4, 16 / 4, 32) = 4 slices
splitk("nn_splitk", 5000, 2048, 128, FALLBACK, ldc=2056)  # the ragged form does not split (and M N > 2^22: no workspace offered)
# TN (Kc, M, N) -> tn(M, N, Kc): the 8-wave K-major kernel, 192-row tile for M <= 192, else 256 (choose_tile answers 0 for all three: 128 x 128 wins or M, N < 192)
for beta in (0, 1):
    tn(64, 200, 128, plan(STAGGER, 192, 1), beta)
    tn(1001, 328, 640, plan(STAGGER, 256, 8), beta)           # 4 x 2 tiles; beta = 1: 10 K tiles, no slice of 16
tn(256, 256, 4096, plan(STAGGER, 256, 1), 0)
tn(256, 256, 4096, plan(STAGGER, 256, 4, sk=4, finish="atomics"), 1)   # tiles x sk x 2 <= 32 and 64 / (2 sk) >= 16: sk = 4
# TN_QUAD under gemm_set_quad(2)
for beta in (0, 1):
    tn(192, 256, 128, plan(QUAD, 192, 1), beta, quad=2)
    tn(256, 512, 192, plan(QUAD, 256, 2), beta, quad=2)
# TN_SPLITK: 6 quad tiles over 32 K tiles -> min(256 / 6, 32 / 8) = 4 slices; 3 x 2 ragged 8-wave tiles over 101 K tiles -> min(42, 12) = 12 slices
splitk("tn_splitk", 512, 768, 2048, ws_plan(QUAD, 256, 6, 4, 512 * 768, "f32"))
splitk("tn_splitk", 520, 264, 6464, ws_plan(STAGGER, 256, 6, 12, 520 * 264, "f32"))
# TN_PAIR: (768 + 256) / 256 x 2 = 8 tiles over 16 K tiles -> 2 slices; one reduce pass per output
pair(768, 256, 512, 1024, ws_plan(QUAD, 256, 8, 2, 1024 * 512, "f32", rgrid=384, rgrid2=128))
# TN_MULTI: 2 + 3 = 5 tiles over 32 K tiles -> 4 slices
multi([(512, 256), (256, 768)], 2048, ws_plan(QUAD, 256, 5, 4, 512 * 256 + 256 * 768, "multi"))
# NT_SPLITK: 3 x 2 tiles of 320 rows over 128 K tiles -> 16 slices; M < 320 falls back (to the 128 x 128 kernel); 2 tiles over 64 K tiles -> 8 slices, ldc = 784
splitk("nt_splitk", 704, 512, 8192, ws_plan(STAGGER, 320, 6, 16, 704 * 512, "bf16"), ldc=520)
splitk("nt_splitk", 100, 300, 640, FALLBACK, ldc=312)
nt(100, 300, 640, plan(SMALL, 128, 3), ldc=312)
splitk("nt_splitk", 640, 256, 4096, ws_plan(STAGGER, 320, 2, 8, 640 * 256, "bf16"), ldc=784)
# the GELU sweep: 34 193 values along N
nt_exact(64, 34304, 128, "gelu", plan(SMALL, 128, 268), tile=0)
nt_exact(64, 34304, 128, "gelu", plan(STAGGER, 256, 134), tile=256)
nt_exact(256, 268 * 256, 128, "gelu", plan(PERSIST, 256, 256), tile=256)      # 268 whole tiles in one tile row

# ================================================================================================ tests/test_gpu_kernels.py
# test_gemm_nt_plain (those not listed above)
for f32 in (0, 1):
    nt(128, 128, 64, plan(SMALL, 128, 1), f32=f32, ldc=128)
    nt(256, 384, 128, plan(SMALL, 128, 6), f32=f32, ldc=384)       # N % 256 != 0: no quad tile; 6 small blocks (50923) before 4 of 192 rows (60779)
    nt(200, 136, 72, plan(SMALL, 128, 4), f32=f32, ldc=136)
    nt(1024, 2048, 512, plan(SMALL, 128, 128), f32=f32, ldc=2048)  # 32 quad tiles < 128; 128 small blocks in one round
    nt(136, 1001, 256, plan(SMALL, 128, 16), f32=f32, ldc=1001)
    nt(8, 384, 32, plan(SMALL, 128, 3), f32=f32, ldc=384)
    nt(40, 64, 2056, plan(SMALL, 128, 1), f32=f32, ldc=64)
# test_gemm_large_tile_kernels: forced tiles, every epilogue
for (M, N, K), grids in (((640, 512, 256), {192: 8, 256: 6, 320: 4, 0: 20}), ((700, 1001, 192), {192: 16, 256: 12, 320: 12, 0: 48}),
                         ((1280, 2048, 2048), {192: 56, 256: 40, 320: 32, 0: 160}), ((333, 260, 128), {192: 4, 256: 4, 320: 4, 0: 9})):
    for tile, grid in grids.items():
        for epi, f32, beta, ldc in ((NONE, 0, 0, up(N, 8)), (BIAS, 1, 0, N), (GELU, 0, 0, up(N, 8)), (DGELU, 0, 0, up(N, 8)), (NONE, 1, 1, N)):
            nt(M, N, K, plan(STAGGER, tile, grid) if tile else plan(SMALL, 128, grid), epi, f32, beta, ldc=ldc, tile=tile)
# test_gemm_persistent_blocks_every_epilogue: plain bf16, bias fp32, GELU, GELU', beta = 1; then the same with gemm_set_persist(0)
FIVE = ((NONE, 0, 0), (BIAS, 1, 0), (GELU, 0, 0), (DGELU, 0, 0), (NONE, 1, 1))
for (M, N, K), tiles in (((5120, 8192, 128), 512), ((5120, 8192, 192), 512), ((10240, 8192, 320), 1024)):
    # whole 320-row tiles in 2 (4) persistent rounds: 2 x 81920 x 0.9 against 3 x 65536 x 0.9 (4 x 81920 ties 5 x 65536: the larger tile); too many tiles for the quad kernel
    for epi, f32, beta in FIVE:
        nt(M, N, K, plan(PERSIST, 320, 256), epi, f32, beta, ldc=N)
        nt(M, N, K, plan(STAGGER, 320, tiles), epi, f32, beta, ldc=N, persist=0)
for persist in (1, 0):
    # 10 x 24 = 240 and 20 x 10 = 200 whole 256-row tiles: ONE round, so not the persistent form whatever the switch; the plain call (256 <= 256 rows a round, bf16)
    # goes to the quad kernel, 4 K tiles on the asm loop, 5 on the C++ one
    kw = {} if persist else dict(persist=0)
    nt(2560, 6144, 256, plan(QUAD, 256, 240, asm=1), ldc=6144, **kw)
    nt(5120, 2560, 320, plan(QUAD, 256, 200), ldc=2560, **kw)
    for epi, f32, beta in FIVE[1:]:
        nt(2560, 6144, 256, plan(STAGGER, 256, 240), epi, f32, beta, ldc=6144, **kw)
        nt(5120, 2560, 320, plan(STAGGER, 256, 200), epi, f32, beta, ldc=2560, **kw)
# test_gemm_tn_kmajor (Kc, M, N): beta = 0 then 1
tn(192, 256, 256, plan(STAGGER, 192, 1), 0), tn(192, 256, 256, plan(STAGGER, 192, 1), 1)
tn(2048, 2048, 1280, plan(STAGGER, 256, 64), 0), tn(2048, 2048, 1280, plan(STAGGER, 256, 64), 1)      # 64 quad tiles < 128: the 8-wave kernel
tn(6144, 2048, 2560, plan(QUAD, 192, 256), 0), tn(6144, 2048, 2560, plan(QUAD, 192, 256), 1)          # 256 tiles of 192 rows: one round x 192 before 192 tiles x 256
tn(320, 8192, 192, plan(STAGGER, 256, 64), 0), tn(320, 8192, 192, plan(STAGGER, 256, 64), 1)
tn(512, 512, 10240, plan(STAGGER, 256, 4), 0)
tn(512, 512, 10240, plan(STAGGER, 256, 32, sk=8, finish="atomics"), 1)                                  # 4 tiles x 8 = 32 blocks, 20 K tiles a slice
tn(300, 260, 4096, plan(STAGGER, 256, 4), 0)
tn(300, 260, 4096, plan(STAGGER, 256, 16, sk=4, finish="atomics"), 1)
# test_gemm_tn_splitk_workspace (Kc, M, N) (those not listed above)
splitk("tn_splitk", 2048, 2048, 10240, ws_plan(QUAD, 256, 64, 4, 2048 * 2048, "f32"))
splitk("tn_splitk", 256, 256, 4096, ws_plan(QUAD, 256, 1, 8, 256 * 256, "f32"))                          # 64 K tiles: 8 slices of 8
splitk("tn_splitk", 2048, 2048, 256, FALLBACK)
splitk("tn_splitk", 304, 264, 1024, ws_plan(STAGGER, 256, 4, 2, 304 * 264, "f32"))
splitk("tn_splitk", 768, 768, 24576, ws_plan(QUAD, 256, 9, 28, 768 * 768, "f32"))                        # 256-row tiles where they are whole: 9, not 12 of 192
splitk("tn_splitk", 3072, 768, 24576, ws_plan(QUAD, 256, 36, 7, 3072 * 768, "f32"))
splitk("tn_splitk", 768, 2304, 24576, ws_plan(QUAD, 256, 27, 9, 768 * 2304, "f32"))
for beta in (0, 1):   # the fallbacks land on udm_gemm_tn_bf16
    tn(2048, 2048, 256, plan(STAGGER, 256, 64), beta)
# test_gemm_quad_asm_k_loop_is_bit_identical: gemm_set_quad(2), asm on / off; 5 K tiles never take the asm loop
for (M, N, K, epi), (rows, grid, takes) in (((640, 512, 256, NONE), (320, 4, 1)), ((640, 256, 1024, BIAS), (320, 2, 1)), ((512, 512, 512, NONE), (256, 4, 1)),
                                            ((1024, 256, 256, BIAS), (256, 4, 1)), ((640, 512, 320, NONE), (320, 4, 0))):
    for asm in (1, 0):
        nt(M, N, K, plan(QUAD, rows, grid, asm=takes and asm), epi, quad=2, asm=asm)
# test_gemm_tn_pair_equals_two_launches (M0, M1, N, Kc) and its two plain launches under gemm_set_quad(2)
pair(6144, 2048, 2048, 10240, plan(QUAD, 256, 256))               # 256 tiles: the chip once, no split
pair(256, 256, 256, 128, plan(QUAD, 256, 2))
pair(2304, 768, 768, 24576, ws_plan(QUAD, 256, 36, 7, 3072 * 768, "f32", rgrid=1728, rgrid2=576))
for beta in (0, 1):
    tn(6144, 2048, 10240, plan(QUAD, 192, 256), beta, quad=2), tn(2048, 2048, 10240, plan(QUAD, 256, 64), beta, quad=2)
    tn(768, 512, 1024, plan(QUAD, 192, 8), beta, quad=2), tn(256, 512, 1024, plan(QUAD, 256, 2), beta, quad=2)
    tn(256, 256, 128, plan(QUAD, 256, 1), beta, quad=2)
    tn(2304, 768, 24576, plan(QUAD, 192, 36), beta, quad=2), tn(768, 768, 24576, plan(QUAD, 192, 12), beta, quad=2)
# test_gemm_tn_multi_equals_separate_launches
multi([(2304, 768), (768, 768), (3072, 768), (768, 3072)], 24576, ws_plan(QUAD, 256, 108, 2, 9216 * 768, "multi"))   # 108 tiles: two slices fill 216 CUs
multi([(256, 256)], 1024, ws_plan(QUAD, 256, 1, 2, 65536, "multi"))
multi([(1024, 4096)], 1024, ws_plan(QUAD, 256, 64, 2, 1024 * 4096, "multi"))    # (the test's last call: its output is not contiguous, which the wrapper refuses)
# test_gemm_tn_pair_falls_back_when_quad_kernels_are_off
pair(768, 256, 512, 1024, NOT_OK, quad=0)
pair(6144, 2048, 2048, 2560, NOT_OK, quad=0)
splitk("tn_splitk", 256, 512, 1024, ws_plan(STAGGER, 256, 2, 2, 256 * 512, "f32"), quad=0)      # out-proj side: few tiles -> gemm_tn_splitk on the 8-wave kernel
splitk("tn_splitk", 768, 512, 1024, ws_plan(STAGGER, 256, 6, 2, 768 * 512, "f32"), quad=0)
splitk("tn_splitk", 2048, 2048, 2560, ws_plan(STAGGER, 256, 64, 4, 2048 * 2048, "f32"), quad=0)
tn(6144, 2048, 2560, plan(STAGGER, 192, 256), 0, quad=0)         # one round either way: 256 tiles of 192 rows (52852) before 192 of 256 rows (65536)
# test_gemm_nt_quad_one_wave_per_simd_every_epilogue: gemm_set_quad(2), then (0)
FIVE_Q = ((NONE, 0), (NONE, 1), (BIAS, 0), (GELU, 0), (DGELU, 0))
for (M, N, K), (rows, grid, asm), small in (((512, 512, 128), (256, 4, 0), 16), ((512, 256, 192), (256, 2, 0), 8), ((768, 512, 448), (192, 8, 0), 24),
                                            ((384, 256, 256), (192, 2, 0), 6), ((1024, 768, 1024), (256, 12, 1), 48), ((640, 512, 320), (320, 4, 0), 20),
                                            ((2560, 2048, 2048), (256, 80, 1), 320)):
    for epi, f32 in FIVE_Q:
        nt(M, N, K, plan(QUAD, rows, grid, asm=asm), epi, f32, ldc=N, quad=2)
        nt(M, N, K, plan(SMALL, 128, small), epi, f32, ldc=N, quad=0)      # the 8-wave side of the comparison: every one of these is one round of 128 x 128 blocks
# test_gemm_tn_quad_one_wave_per_simd (Kc, M, N): gemm_set_quad(2) beta 0 / 1, gemm_set_quad(0), gemm_tn_splitk under (2) where M % 256 == 0
for (K, M, N), (rows, grid), (rows0, grid0) in (((128, 256, 256), (256, 1), (256, 1)), ((192, 512, 512), (256, 4), (256, 4)), ((256, 512, 256), (256, 2), (256, 2)),
                                               ((448, 256, 512), (256, 2), (256, 2)), ((1024, 768, 512), (192, 8), (256, 6)), ((320, 384, 256), (192, 2), (256, 2)),
                                               ((640, 192, 512), (192, 2), (192, 2)), ((10240, 2048, 2048), (256, 64), (256, 64)), ((2560, 8192, 2048), (256, 256), (256, 256))):
    for beta in (0, 1):
        tn(M, N, K, plan(QUAD, rows, grid), beta, quad=2)
    tn(M, N, K, plan(STAGGER, rows0, grid0), 0, quad=0)
for M, N, K in ((256, 256, 128), (512, 512, 192), (512, 256, 256), (256, 512, 448), (8192, 2048, 2560)):
    splitk("tn_splitk", M, N, K, FALLBACK, quad=2)                 # fewer than 16 K tiles, or 256 tiles already
splitk("tn_splitk", 768, 512, 1024, ws_plan(QUAD, 256, 6, 2, 768 * 512, "f32"), quad=2)
splitk("tn_splitk", 2048, 2048, 10240, ws_plan(QUAD, 256, 64, 4, 2048 * 2048, "f32"), quad=2)
# test_gemm_nn_dgrad_from_forward_shadow: gemm_nn, then gemm_nt under gemm_set_quad(2) (same tile; the NT form has the asm loop on 256- / 320-row tiles)
for (M, N, K), (rows, grid, asm) in (((192, 256, 128), (192, 1, 0)), ((256, 512, 192), (256, 2, 0)), ((320, 256, 256), (320, 1, 1)), ((640, 512, 448), (320, 4, 0)),
                                     ((768, 256, 1024), (192, 4, 0)), ((10240, 2048, 2048), (320, 256, 1)), ((1280, 2048, 6144), (256, 40, 1)), ((2560, 2048, 8192), (256, 80, 1))):
    nn(M, N, K, plan(QUAD, rows, grid))
    nt(M, N, K, plan(QUAD, rows, grid, asm=asm), ldc=N, quad=2)
# test_gemm_nn_ragged_last_tile_row: gemm_nn; gemm_nt plain and bias in auto mode; both under gemm_set_quad(0)
for (M, N, K), grid, auto, off in (((9216, 2048, 2048), 232, plan(RAGGED, 320, 232), plan(STAGGER, 320, 232)), ((9216, 2048, 6144), 232, plan(RAGGED, 320, 232), plan(STAGGER, 320, 232)),
                                   ((5000, 2048, 512), 128, plan(STAGGER, 192, 216), plan(STAGGER, 192, 216)), ((4100, 2560, 256), 130, plan(STAGGER, 192, 220), plan(STAGGER, 192, 220)),
                                   ((10248, 2048, 128), 264, plan(STAGGER, 192, 432), plan(STAGGER, 192, 432))):
    nn(M, N, K, plan(RAGGED, 320, grid))       # 320-row tiles that fill at least half the chip, fewer rounds x rows than any whole tile height (none divides 4100 or 10248)
    for epi in (NONE, BIAS):
        nt(M, N, K, auto, epi, ldc=N)          # only where choose_tile itself picks 320-row tiles for ONE round does NT take the ragged quad form
        nt(M, N, K, off, epi, ldc=N, quad=0)
# test_gemm_single_round_shapes_split_by_rows_when_cus_are_held: M = 10240, d = 2048, dff = 8192; all CUs, then 248 / 240 / 224 (kernels._row_split cuts the rows)
nn(10240, 2048, 8192, plan(QUAD, 320, 256))
tn(8192, 2048, 10240, plan(QUAD, 256, 256)), tn(2048, 8192, 10240, plan(QUAD, 256, 256)), tn(6144, 2048, 10240, plan(QUAD, 192, 256))
nt(10240, 2048, 8192, plan(QUAD, 320, 256, asm=1), BIAS, ldc=2048)
for cus, nn_rest, tn_rest, tn2_sk, q_main, q_rest in (
        (248, (320, 8, 31), (8, 20), 7, 5952, (192, 192, 8, 20)),      # rest: (rows, tiles, slices); qkv rest: (M, tile rows, tiles, slices)
        (240, (320, 16, 15), (16, 15), 7, 5760, (384, 192, 16, 15)),
        (224, (256, 40, 5), (32, 7), 7, 5376, (768, 256, 24, 9))):
    g = cus // 8
    nn(g * 320, 2048, 8192, plan(QUAD, 320, cus), cus=cus)                                                    # the tile rows that fit the CUs left: one round
    rows, tiles, sk = nn_rest
    splitk("nn_splitk", 10240 - g * 320, 2048, 8192, ws_plan(QUAD, rows, tiles, sk, (10240 - g * 320) * 2048, "bf16"), cus=cus)   # cus / tiles slices (128 K tiles / 4 allow 32)
    tn(g * 256, 2048, 10240, plan(QUAD, 256, cus), cus=cus)
    tiles, sk = tn_rest
    splitk("tn_splitk", 8192 - g * 256, 2048, 10240, ws_plan(QUAD, 256, tiles, sk, (8192 - g * 256) * 2048, "f32"), cus=cus)      # at most 160 / 8 = 20 slices
    tn(1792, 8192, 10240, plan(QUAD, 256, 224), 1, cus=cus)                                                   # 7 of the 8 tile rows at every cap (32 tiles a row)
    splitk("tn_splitk", 256, 8192, 10240, ws_plan(QUAD, 256, 32, tn2_sk, 256 * 8192, "f32"), cus=cus)
    nt(g * 320, 2048, 8192, plan(QUAD, 320, cus, asm=1), BIAS, ldc=2048, cus=cus)
    nt(10240 - g * 320, 2048, 8192, plan(SMALL, 128, -(-(10240 - g * 320) // 128) * 16), BIAS, ldc=2048, cus=cus)  # the leftover rows on small tiles
    tn(q_main, 2048, 10240, plan(QUAD, 192, cus), cus=cus)
    M, rows, tiles, sk = q_rest
    splitk("tn_splitk", M, 2048, 10240, ws_plan(QUAD, rows, tiles, sk, M * 2048, "f32"), cus=cus)
# test_gemm_nt_splitk_bf16_output (those not listed above)
splitk("nt_splitk", 5120, 2048, 48512, ws_plan(STAGGER, 320, 128, 2, 5120 * 2048, "bf16"))   # the head dgrad: 128 tiles, two slices of 379 K tiles
splitk("nt_splitk", 5056, 2048, 4096, ws_plan(STAGGER, 320, 128, 2, 5056 * 2048, "bf16"))
splitk("nt_splitk", 5120, 2048, 192, FALLBACK)
nt(5120, 2048, 192, plan(STAGGER, 192, 216), ldc=2048)      # 160 quad tiles of 256 rows cost a round of 256, choose_tile's 216 tiles of 192 rows one of 192

# ================================================================================================ unidisc_amd/dit.py on all rows (tests/test_gpu_fullwidth_oracle.py)
# d = 2048 (K or N = 2048 / 6144 / 8192): qkv, out-proj, mlp.0 + GELU, mlp.2 + bias, the GELU' dgrad; the three dgrads from the forward shadow; pair + two plain wgrads
for M, qkv, out, fc1, fc2, nn_plan in (
        (10240, plan(PERSIST, 320, 256), plan(QUAD, 320, 256, asm=1), plan(PERSIST, 320, 256), plan(QUAD, 320, 256, asm=1), plan(QUAD, 320, 256)),
        (2560, plan(QUAD, 256, 240, asm=1), plan(SMALL, 128, 320), plan(STAGGER, 320, 256), plan(SMALL, 128, 320), plan(QUAD, 256, 80)),
        (9216, plan(PERSIST, 256, 256), plan(RAGGED, 320, 232), plan(PERSIST, 256, 256), plan(RAGGED, 320, 232), plan(RAGGED, 320, 232))):
    nt(M, 6144, 2048, qkv), nt(M, 2048, 2048, out), nt(M, 8192, 2048, fc1, GELU), nt(M, 2048, 8192, fc2, BIAS), nt(M, 8192, 2048, fc1, DGELU)
    for K in (6144, 2048, 8192):
        nn(M, 2048, K, nn_plan)
    pair(6144, 2048, 2048, M, plan(QUAD, 256, 256))
    tn(8192, 2048, M, plan(QUAD, 256, 256)), tn(2048, 8192, M, plan(QUAD, 256, 256))
# d = 768, M = 1536: every forward GEMM is one round of 128 x 128 blocks; four wgrads in one launch of 108 tiles x 2 slices
nt(1536, 2304, 768, plan(SMALL, 128, 216)), nt(1536, 768, 768, plan(SMALL, 128, 72)), nt(1536, 3072, 768, plan(SMALL, 128, 288), GELU)
nt(1536, 768, 3072, plan(SMALL, 128, 72), BIAS), nt(1536, 3072, 768, plan(SMALL, 128, 288), DGELU)
for K in (2304, 768, 3072):
    nn(1536, 768, K, plan(QUAD, 192, 24))
multi([(768, 3072), (3072, 768), (768, 768), (2304, 768)], 1536, ws_plan(QUAD, 256, 108, 2, 9216 * 768, "multi"))
# d = 256, M = 1024 / 512
for M in (1024, 512):
    nt(M, 768, 256, plan(SMALL, 128, M // 128 * 6)), nt(M, 256, 256, plan(SMALL, 128, M // 128 * 2)), nt(M, 1024, 256, plan(SMALL, 128, M // 128 * 8), GELU)
    nt(M, 256, 1024, plan(SMALL, 128, M // 128 * 2), BIAS), nt(M, 1024, 256, plan(SMALL, 128, M // 128 * 8), DGELU)
    for K in (768, 256, 1024):
        nn(M, 256, K, plan(QUAD, 256, M // 256))
multi([(256, 1024), (1024, 256), (256, 256), (768, 256)], 1024, ws_plan(QUAD, 256, 12, 2, 3 * 262144, "multi"))
multi([(256, 1024), (1024, 256), (256, 256), (768, 256)], 512, NOT_OK)       # 8 K tiles: no two slices of 8 -> the four plain calls, which do not split either
for M, N in ((256, 1024), (1024, 256), (256, 256), (768, 256)):
    splitk("tn_splitk", M, N, 512, FALLBACK)
    tn(M, N, 512, plan(STAGGER, 256, (M // 256) * (N // 256)))

# ================================================================================================ the measured choices gemm_plan.h records
nt(24576, 3072, 768, plan(PERSIST, 256, 256), GELU), nt(24576, 3072, 768, plan(PERSIST, 256, 256), DGELU), nt(24576, 2304, 768, plan(PERSIST, 256, 256))
nt(9216, 8192, 2048, plan(PERSIST, 256, 256), GELU)       # 1152 tiles: 5 persistent rounds of 256 (x 0.9) against 6 of 192
nt(9216, 6144, 2048, plan(PERSIST, 256, 256))             # 864 tiles: 4 rounds of 256 against 3 of ragged 320
nt(9216, 2048, 2048, plan(RAGGED, 320, 232))

# ================================================================================================ one case on each side of every gate (tagged extra: no GPU test runs them)
X = dict(extra=True)
# K % 64 and K < 128: the forced tile holds only for K the LDS-DMA kernels take
nt(1024, 1024, 128, plan(STAGGER, 256, 16), tile=256, **X), nt(1024, 1024, 64, plan(SMALL, 128, 64), tile=256, **X), nt(1024, 1024, 136, plan(SMALL, 128, 64), tile=256, **X)
# M, N < 192: two rounds of 128 x 128 blocks (88562) against one of 192-row tiles (52852) - but not below 192
nt(192, 65536, 2048, plan(STAGGER, 192, 256), quad=0, **X), nt(184, 65536, 2048, plan(SMALL, 128, 1024), quad=0, **X)
nt(49152, 192, 2048, plan(STAGGER, 192, 256), quad=0, **X), nt(49152, 184, 2048, plan(SMALL, 128, 768), quad=0, **X)
# 256 / 257 tiles for the persistent form
nt(4096, 4096, 256, plan(STAGGER, 256, 256), tile=256, **X), nt(65792, 256, 128, plan(PERSIST, 256, 256), tile=256, **X)
# ldc / ldaux alignment of the wide epilogue: bf16 C % 8, fp32 C % 4, aux % 8
nt(4352, 4096, 128, plan(STAGGER, 256, 272), ldc=4100, tile=256, **X), nt(4352, 4096, 128, plan(PERSIST, 256, 256), f32=1, ldc=4100, tile=256, **X)
nt(4352, 4096, 128, plan(STAGGER, 256, 272), f32=1, ldc=4098, tile=256, **X), nt(4352, 4096, 128, plan(STAGGER, 256, 272), GELU, ldc=4104, ldaux=4100, tile=256, **X)
# every epilogue and output type of the persistent and the one-block-per-tile form on forced 256- and 320-row tiles (test_nt_persistent_wide runs four of the seven)
for tile, M in ((256, 4352), (320, 5440)):
    for v in ("none_f32", "bias_bf16", "dgelu_f32"):
        nt_exact(M, 4096, 128, v, plan(PERSIST, tile, 256), tile=tile, **X)
nt(4352, 4096, 128, plan(PERSIST, 256, 224), tile=256, cus=224, **X)     # a CU cap of 224: that many persistent blocks
# 127 / 128 / 256 / 257 quad tiles in auto mode (N = 256: one tile column)
nt(32512, 256, 2048, plan(SMALL, 128, 508), **X), nt(32768, 256, 2048, plan(QUAD, 256, 128, asm=1), **X), nt(65536, 256, 2048, plan(QUAD, 256, 256, asm=1), **X)
nt(65792, 256, 2048, plan(RAGGED, 320, 206), **X)          # 257 whole tiles are refused; 206 ragged 320-row tiles are one round
# GELU epilogues, beta != 0 and fp32 output with an epilogue keep the 8-wave kernel where the plain bf16 call takes the quad one (256 tiles of 320 rows: not persistent)
nt(10240, 2048, 8192, plan(STAGGER, 320, 256), GELU, **X), nt(10240, 2048, 8192, plan(STAGGER, 320, 256), DGELU, **X)
nt(10240, 2048, 8192, plan(STAGGER, 320, 256), NONE, 1, 1, **X), nt(10240, 2048, 8192, plan(STAGGER, 320, 256), BIAS, 1, **X)
nt(10240, 2048, 8192, plan(QUAD, 320, 256, asm=1), NONE, 1, **X), nt(10240, 2048, 8192, plan(STAGGER, 320, 256), ldc=2050, **X)    # (ldc % 4 for the quad epilogue)
# the generated K loop under the GELU / GELU' epilogue on 320-row tiles, and UDM_QUAD_ASM = 2
nt(640, 512, 256, plan(QUAD, 320, 4, asm=1), GELU, quad=2, **X), nt(640, 512, 256, plan(QUAD, 320, 4, asm=1), DGELU, quad=2, **X)
nt(640, 512, 256, plan(QUAD, 320, 4, asm=2), quad=2, asm=2, **X)
# slice depth: 8 K tiles (TN) against 4 (NN) on 16 K tiles; the 32-slice cap; a workspace one float too small
splitk("tn_splitk", 768, 256, 1024, ws_plan(QUAD, 256, 3, 2, 768 * 256, "f32"), **X)
splitk("tn_splitk", 256, 256, 24576, ws_plan(QUAD, 256, 1, 32, 65536, "f32"), **X)
splitk("tn_splitk", 512, 768, 2048, FALLBACK, ws=4 * 512 * 768 - 1, **X)
splitk("nt_splitk", 704, 512, 8192, FALLBACK, ldc=520, ws=16 * 704 * 512 - 1, **X)
splitk("nn_splitk", 768, 256, 1024, FALLBACK, ldc=264, ws=4 * 768 * 256 - 1, **X)
splitk("tn_splitk", 512, 768, 2048, FALLBACK, ldc=776, **X)                       # C not contiguous
pair(768, 256, 512, 1024, plan(QUAD, 256, 8), ws=2 * 1024 * 512 - 1, **X)         # the pair then launches unsplit
pair(768, 256, 512, 1024, plan(QUAD, 256, 8), contiguous=0, **X)
pair(768, 200, 512, 1024, NOT_OK, **X)
multi([(512, 256), (256, 768)], 2048, NOT_OK, ws=4 * 327680 - 1, **X)
# tiles > 128 for the multi form
multi([(2048, 4096)], 24576, ws_plan(QUAD, 256, 128, 2, 2048 * 4096, "multi"), **X), multi([(3072, 3072)], 24576, NOT_OK, **X)
# the atomics split of udm_gemm_tn_bf16: tiles x sk x 2 <= 32
tn(1024, 1024, 8192, plan(STAGGER, 256, 32, sk=2, finish="atomics"), 1, **X), tn(1280, 1024, 8192, plan(STAGGER, 256, 20), 1, **X)
# the K-major 8-wave kernel on 320-row tiles; UDM_QUAD_RAGGED = 0; udm_gemm_nn_ok's refusals
tn(640, 512, 256, plan(STAGGER, 320, 4), tile=320, **X), tn(640, 512, 256, plan(STAGGER, 192, 8), tile=192, **X)
nn(9216, 2048, 2048, plan(QUAD, 192, 384), ragged=0, **X), nn(5000, 2048, 128, NOT_OK, ragged=0, **X)
nn(200, 256, 128, NOT_OK, **X), nn(192, 384, 128, NOT_OK, **X), nn(192, 256, 160, NOT_OK, **X), nn(192, 256, 128, NOT_OK, quad=0, **X)

SPLIT_ENTRIES = ("nt_splitk", "tn_splitk", "nn_splitk", "tn_pair", "tn_multi")
CAPS = (0, 224, 128)


def _ask(K, entry, args):
    """what the wrapper of unidisc_amd/kernels.py offers for this call (GEMM_WS reads the CU cap kernels.gemm_set_cus keeps in _CUS)"""
    if entry == "tn_pair":
        return K.GEMM_WS["gemm_tn_pair"](*args[:4])
    if entry == "tn_multi":
        return K.GEMM_WS["gemm_tn_multi"](list(zip(args[2::2], args[3::2])), args[0])
    return K.GEMM_WS["gemm_" + entry](*args[:3])


def _line(entry, name, env, args):
    return f"{entry} {name} {env['cus']} {env['quad']} {env['persist']} {env['tile']} {env['ragged']} {env['asm']} {len(args)} " + " ".join(str(a) for a in args) + "\n"


def _with_ws(entry, args, ws):
    i = dict(tn_pair=5, tn_multi=1).get(entry, 4)
    return args[:i] + (ws,) + args[i + 1:]


def slice_rule_inputs():
    """(tiles, K, depth, cus) of every split entry of the table as its entry point counts them, and the edges of the rule"""
    out = {(1, 24576, 8, 256), (1, 64 * 16, 8, 256), (1, 64 * 15, 8, 256), (128, 8192, 8, 256), (129, 8192, 8, 256), (4, 1024, 4, 256), (4, 1024, 8, 256), (7, 8192, 8, 224), (300, 8192, 8, 256)}
    for entry, args, env, _, _ in CASES.values():
        if entry in ("nt_splitk", "tn_splitk", "nn_splitk"):
            M, N, Kd = args[:3]
            rows = dict(nt_splitk=(320,), tn_splitk=(256, 192), nn_splitk=(192, 256, 320))[entry]
            out |= {(-(-M // r) * -(-N // 256), Kd, 4 if entry == "nn_splitk" else 8, c) for r in rows for c in (256, env["cus"])}
        elif entry == "tn_pair":
            out.add(((args[0] + args[1]) // 256 * (args[2] // 256), args[3], 8, 256))
        elif entry == "tn_multi":
            out.add((sum((m // 256) * (n // 256) for m, n in zip(args[2::2], args[3::2])), args[0], 8, env["cus"]))
    return sorted(t for t in out if t[0] > 0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """build the printer with the host compiler, run it once over the whole table: {case name: {"": plan}}; for the split entry points also the plan under the
    wrapper's ask and under more than any launch needs at each CU cap: {"ask<cap>": plan, "huge<cap>": plan}; and {"slices": {(tiles, K, depth, cus): slices}}"""
    from unidisc_amd import kernels as K
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    lines, asks = [], {}
    saved = K._CUS[0]
    try:
        for name, (entry, args, env, _, _) in CASES.items():
            if entry not in SPLIT_ENTRIES:
                lines.append(_line(entry, name + "|", env, args))
                continue
            for cap in CAPS:
                K._CUS[0] = cap
                asks[name, cap] = _ask(K, entry, args)
                e = dict(env, cus=cap or 256)
                lines.append(_line(entry, f"{name}|ask{cap}", e, _with_ws(entry, args, asks[name, cap])))
                lines.append(_line(entry, f"{name}|huge{cap}", e, _with_ws(entry, args, HUGE)))
            K._CUS[0] = 0 if env["cus"] == 256 else env["cus"]
            ws = args[dict(tn_pair=5, tn_multi=1).get(entry, 4)]
            lines.append(_line(entry, name + "|", env, _with_ws(entry, args, _ask(K, entry, args) if ws == ASK else ws)))
    finally:
        K._CUS[0] = saved
    rule = slice_rule_inputs()
    lines += [_line("slices", f"slices|{i}", ENV, t) for i, t in enumerate(rule)]
    run = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {"slices": {}, "asks": asks}
    for row in run.stdout.splitlines():
        key, *fields = row.split()
        name, kind = key.split("|")
        got = dict(f.split("=") for f in fields)
        if name == "slices":
            out["slices"][rule[int(kind)]] = int(got["splitk"])
        else:
            out.setdefault(name, {})[kind] = got
    assert [n for n in out if n not in ("slices", "asks")] == list(CASES) and len(out["slices"]) == len(rule), "the printer did not answer every case"
    return out


def lds_bytes(family, rows):
    """two stages of an A and a B tile of 64 bf16 columns: 128 + 128 rows of the register-staged kernel, rows + 256 of the others"""
    return 2 * ((128 + 128) if family == SMALL else (rows + 256)) * 64 * 2


@pytest.mark.parametrize("name", list(CASES))
def test_plan(plans, name):
    _, _, env, expect, _ = CASES[name]
    got = plans[name][""]
    if expect == NOT_OK:
        assert got["ok"] == "0", got
        return
    assert got["ok"] == "1", got
    if expect == FALLBACK:
        assert got["fallback"] == "1" and got["grid"] == "0" and got["need"] == "0", got
        return
    assert got["fallback"] == "0", got
    for k, v in expect.items():
        assert got[k] == str(v), (k, v, got)
    assert int(got["lds"]) == lds_bytes(expect["family"], expect["rows"]), got
    tm, tn_ = (int(x) for x in got["tiles"].split("x"))
    assert tm * tn_ * expect["splitk"] == expect["grid"] or (expect["family"] == PERSIST and expect["grid"] == env["cus"] and tm * tn_ > 256), got


def _src(name):
    return open(os.path.join(ROOT, "unidisc_amd", "csrc", name)).read()


EPI_NAMES = dict(NONE=NONE, BIAS=BIAS, BIAS_GELU=GELU, DGELU=DGELU)


def launchable():
    """every GEMM kernel instantiation the dispatchers can launch, read from their source, as
    ("small", epi, out_f32) | ("big", rows, epi, out_f32, tn, persistent) | ("quad", fm, form, epi, out_f32, ragged, asm loop)"""
    out = set()
    g = _src("gemm.hip")
    host = g[g.index("GemmEnv gemm_env_from_environment()"):]
    # the 128 x 128 kernel: launch_gemm<EPI> holds both output types; the entry point's argument check refuses fp32 output with the GELU epilogue
    small = re.findall(r"launch_gemm<UDM_EPI_(\w+)>\(a, p, out_f32, stream\)", host)
    assert len(small) == 4 == host.count("return launch_gemm<") and "EPI_BIAS_GELU needs aux and bf16 output" in host
    out |= {("small", EPI_NAMES[e], f) for e in small for f in (0, 1) if not (EPI_NAMES[e] == GELU and f)}
    # the 8-wave kernel: launch_big<rows> x the (epilogue, output type) list of launch_big, persistent as well for NT rows >= 256; and the explicit K-major / split launches
    body = host[host.index("int launch_big(const GemmArgs& a"):host.index("template <int EPI>\nint launch_gemm")]
    combos = {(EPI_NAMES[e], int(f == "true")) for e, f in re.findall(r"launch_big_t<BMX, UDM_EPI_(\w+), (true|false)>", body)}
    assert len(combos) == 7 == body.count("launch_big_t<")
    assert "if constexpr (!TN && BMX >= 256) {\n    if (p.family == GEMM_PERSIST)" in host
    for rows in {int(r) for r in re.findall(r"return launch_big<(\d+)>\(", host)}:
        out |= {("big", rows, e, f, 0, per) for e, f in combos for per in ((0, 1) if rows >= 256 else (0,))}
    explicit = re.findall(r"launch_big_t<(\d+), UDM_EPI_NONE, true, (true|false)>\(a, p, stream\)", host)
    assert len(explicit) == len(re.findall(r"launch_big_t<\d", host))
    out |= {("big", int(r), NONE, 1, int(t == "true"), 0) for r, t in explicit}
    # the one-wave-per-SIMD kernel: the explicit lists of udm_quad_launch and launch_quad_nt_fm<FM>; the asm loop per `if constexpr` of launch_quad_t
    q = _src("gemm_quad.hip")
    host = q[q.index("int launch_quad_t(const QuadArgs& a0, const GemmPlan& p"):]
    assert "if constexpr (MODE == 0 && !RAGGED && (FM == 4 || FM == 5)) {\n    if (p.asm_loop)" in host
    fms = [int(f) for f in re.findall(r"return launch_quad_nt_fm<(\d)>\(", host)]
    calls = re.findall(r"launch_quad_t<(\d|FM), (true|false|2), UDM_EPI_(\w+), (true|false)(, true)?>\(a, p, stream\)", host)
    assert len(calls) == host.count("launch_quad_t<")
    for fm, mode, e, f, ragged in calls:
        form = {"false": "nt", "true": "tn", "2": "nn"}[mode]
        for m in (fms if fm == "FM" else [int(fm)]):
            asm = (0, 1) if form == "nt" and not ragged and m in (4, 5) else (0,)
            out |= {("quad", m, form, EPI_NAMES[e], int(f == "true"), int(bool(ragged)), a) for a in asm}
    return out


def selected_by(entry, args, got):
    """the instantiation a plan of the table launches"""
    fam, rows, asm = got["family"], int(got["rows"]), int(got["asm"])
    epi, f32 = (args[5], args[6]) if entry == "nt" else (NONE, int(entry not in ("nn", "nt_splitk") or fam not in (QUAD, RAGGED)))
    if entry == "nt_splitk":
        f32 = 1
    if fam == SMALL:
        return ("small", epi, f32)
    if fam in (STAGGER, PERSIST):
        return ("big", rows, epi, f32, int(entry in ("tn", "tn_splitk")), int(fam == PERSIST))
    form = "nt" if entry == "nt" else ("nn" if entry.startswith("nn") else "tn")
    return ("quad", rows // 64, form, epi, f32, int(fam == RAGGED), min(asm, 1))     # (asm = 2 runs the first statement's instance unless the build has the second)


def test_every_instance_has_a_case(plans):
    """The instantiations the plans of the table select are exactly those the dispatchers of gemm.hip / gemm_quad.hip can launch: an instantiation without a case is
    either dead (delete it) or a gap of this table, and a plan that names an instance no dispatcher holds would launch nothing.  The cases tagged `extra` are run by no
    GPU test: what they alone select is what the module docstring names."""
    sel, sel_gpu = set(), set()
    for name, (entry, args, _, expect, extra) in CASES.items():
        if expect in (NOT_OK, FALLBACK):
            continue
        inst = selected_by(entry, args, plans[name][""])
        sel.add(inst)
        if not extra:
            sel_gpu.add(inst)
    can = launchable()
    assert sel == can, (sorted(sel - can), sorted(can - sel))
    no_gpu_test = {("big", 320, NONE, 1, 1, 0)} | {("big", r, e, f, 0, 1) for r in (256, 320) for e, f in ((NONE, 1), (BIAS, 0), (DGELU, 1)) if (r, e) != (320, NONE)} | \
        {("quad", 5, "nt", e, 0, 0, 1) for e in (GELU, DGELU)}
    assert sel - sel_gpu == no_gpu_test, (sorted(sel - sel_gpu - no_gpu_test), sorted(no_gpu_test - (sel - sel_gpu)))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[0] in SPLIT_ENTRIES])
def test_asks_cover_the_plan(plans, name):
    """The workspace unidisc_amd/kernels.py asks `_scratch` for (GEMM_WS) with all CUs and with 224 and 128 of them, against the plan chosen when exactly that much is
    offered: the ask is 0 or covers what the launch writes and the reduction reads, and it is never the ask that keeps a launch off the split - the plan under the ask
    is the plan under any larger buffer (`_scratch` hands over its whole buffer).  Without an ask the wrapper passes no workspace (gemm_tn_multi: does not call), and
    the plan is the plain entry point's, an unsplit pair or no launch.  Asserted for the shapes of the table; ASK_TOO_SMALL would name the exceptions: there are none."""
    entry = CASES[name][0]
    for cap in CAPS:
        ask, at_ask, at_huge = plans["asks"][name, cap], plans[name][f"ask{cap}"], plans[name][f"huge{cap}"]
        assert ask == 0 or ask >= int(at_ask["need"]), (cap, ask, at_ask)
        if name in ASK_TOO_SMALL:
            assert ask and at_ask != at_huge and int(at_huge["need"]) > ask, (cap, ask, at_ask, at_huge)
        elif ask:
            assert at_ask == at_huge, (cap, at_ask, at_huge)
        else:
            assert at_ask["splitk"] == "1" and at_ask["need"] == "0" and (at_ask["fallback"] == "1" or at_ask["ok"] == "0" or entry == "tn_pair"), (cap, at_ask)
            if entry != "nn_splitk":    # (gemm_nn_splitk offers nothing for M N > 2^22 floats, whatever a split would take)
                assert at_huge == at_ask, (cap, at_ask, at_huge)


def test_split_rule_is_one_rule(plans):
    """kernels._splitk_slices and gemm_splitk_slices of the header on the tile counts, depths and CU counts of the table's split entries, and on the rule's edges"""
    from unidisc_amd import kernels as K
    assert len(plans["slices"]) > 50
    for (tiles, Kd, depth, cus), got in plans["slices"].items():
        assert K._splitk_slices(tiles, Kd, depth, cus) == got, (tiles, Kd, depth, cus, got)
    assert plans["slices"][1, 24576, 8, 256] == 32 and plans["slices"][1, 1024, 8, 256] == 2 and plans["slices"][1, 960, 8, 256] == 1
    assert plans["slices"][128, 8192, 8, 256] == 2 and plans["slices"][129, 8192, 8, 256] == 1 and plans["slices"][4, 1024, 4, 256] == 4 and plans["slices"][4, 1024, 8, 256] == 2
