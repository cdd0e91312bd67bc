"""Which instantiation and grid udm_attention_fwd_kv launches: attn_plan_fwd_kv of unidisc_amd/csrc/attention_plan.h, compiled alone with a host compiler
(tests/attention_kv_plan_print.cpp) and asked for the plan of every shape tests/test_gpu_attention_kv_rowwise.py calls, and of the target shapes of
DESIGN.md "Modality KV cache".  Expected numbers are written out below, not computed from the header: instantiation (head dim), 128-query blocks per
(b, h), 64-key tiles of a block's walk, grid, dynamic LDS, workgroups per CU the kernel is compiled for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = {32: 16384, 64: 32768, 128: 65536, 256: 131072}      # K0 | K1 | V0 | V1, 64 keys each
WGS = {32: 2, 64: 2, 128: 2, 256: 1}
# (Lq, Lk) -> (q_tiles, kv_tiles)
TILES = {(48, 560): (1, 9), (77, 333): (1, 6), (129, 193): (2, 4), (8, 72): (1, 2), (128, 640): (1, 10)}

CASES = []   # (name, "D B H Lq Lk", expected dict)


def case(name, B, H, Lq, Lk, D, q_tiles, kv_tiles, grid, grid_ok=1):
    CASES.append((name, f"{D} {B} {H} {Lq} {Lk}",
                  dict(D=D, q_tiles=q_tiles, kv_tiles=kv_tiles, grid=grid, lds=LDS[D], wgs=WGS[D], grid_ok=grid_ok)))


# ---- tests/test_gpu_attention_kv_rowwise.py: (B, H) = (2, 2), every shape x head dim
for (Lq, Lk), (qt, kt) in TILES.items():
    for D in (32, 64, 128, 256):
        case(f"rowwise_2x2x{Lq}x{Lk}x{D}", 2, 2, Lq, Lk, D, qt, kt, 4 * qt)
case("rowwise_3x5x129x193x64", 3, 5, 129, 193, 64, 2, 4, 30)   # B H = 15
# (the lse = NULL cases and the wrapper case run (2, 2, 77, 333); the argument-error case's valid call (2, 2, 48, 560, 64): both in the table above)
# ---- the target shapes (DESIGN.md "Modality KV cache"): text steps of 1.4 B at B = 8 and B = 1, of UniDisc-S at B = 64
case("target_1p4b_B8", 8, 16, 256, 1280, 128, 2, 20, 256)
case("target_1p4b_B1", 1, 16, 256, 1280, 128, 2, 20, 32)
case("target_small_B64", 64, 12, 128, 384, 64, 1, 6, 768)
case("target_xxl_B1", 1, 16, 256, 1280, 256, 2, 20, 32)
# ---- edges: one query, one key, Lq just over a block, the grid limit
case("edge_1x1", 1, 1, 1, 1, 32, 1, 1, 1)
case("edge_Lq_129", 1, 8, 129, 129, 128, 2, 3, 16)
case("edge_grid_2^31-8", (1 << 28) - 1, 8, 128, 64, 64, 1, 1, (1 << 31) - 8)
case("edge_grid_2^31", 1 << 28, 8, 128, 64, 64, 1, 1, 0, grid_ok=0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("attention_kv_plan") / "attention_kv_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "attention_kv_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    names = [n for n, _, _ in CASES]
    assert len(set(names)) == len(names)
    run = subprocess.run([exe], input="".join(f"{line} {name}\n" for name, line, _ in CASES), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        name, *fields = ln.split()
        out[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return out


def test_every_case_was_planned(plans):
    assert set(plans) == {n for n, _, _ in CASES}


@pytest.mark.parametrize("name,line,expect", CASES, ids=[c[0] for c in CASES])
def test_plan(plans, name, line, expect):
    assert plans[name] == expect, (line, plans[name], expect)
