"""How the skinny GEMM of a decode step splits K over workgroups: unidisc_amd/csrc/skinny_plan.h, compiled alone with a host compiler
(tests/skinny_plan_print.cpp), against kernels.skinny_ws_elems and against the restatement below of what udm_gemm_skinny_bf16 computed inline before the
header existed.  M in {1, 8, 64, 65, 128} on the five GEMM shapes of UniDisc-S and of the 1.4 B model and on the test models' decode shapes; workspaces:
none, too small for one slab, two slabs, what skinny_ws_elems asks for, and more.  With at least skinny_ws_elems(M, N, K) elements S and kslice do not
depend on M: the row halves of a 65 .. 128-row call are split as calls on those rows are."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 8, 64, 65, 128]
# (N, K): qkv, out-proj, MLP up, MLP down, vocabulary head - 1.4 B, UniDisc-S, the test models (d = 64), and the shapes of tests/gemm_ref64.SKINNY_NK
SHAPES = [(6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192), (48385, 2048), (2304, 768), (768, 768), (3072, 768), (768, 3072), (40193, 768),
          (192, 64), (64, 64), (256, 64), (64, 256), (65, 64), (16384, 128), (16352, 256)]


def expected(M, N, K, ws):
    """(nblk, S, kslice) of the entry point's rule; ws None: no workspace"""
    nblk = (N + 31) // 32
    S = 1
    if ws is not None and nblk < 512:
        S = (512 + nblk // 2) // nblk
        S = min(S, K // 128)
        S = min(S, 32)
        S = min(S, ws // (M * N))
        S = max(S, 1)
    kslice = ((K + S - 1) // S + 31) // 32 * 32
    return nblk, (K + kslice - 1) // kslice, kslice


def workspaces(M, N, K):
    from unidisc_amd import kernels as Kn

    need = Kn.skinny_ws_elems(M, N, K)
    return [None, 0, M * N - 1, 2 * M * N, need, need + 1, 40 * M * N]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("skinny_plan") / "skinny_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "skinny_plan_print.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    cases = sorted({(M, N, K, -1 if ws is None else ws) for M in ROWS for N, K in SHAPES for ws in workspaces(M, N, K)})
    run = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    out = {}
    for row in run.stdout.splitlines():
        f = {k: int(v) for k, v in (kv.split("=") for kv in row.split())}
        out[(f["M"], f["N"], f["K"], f["ws"])] = f
    assert sorted(out) == cases
    return out


def test_the_plan_is_the_entry_points_rule(plans):
    for (M, N, K, ws), got in plans.items():
        assert (got["nblk"], got["S"], got["kslice"]) == expected(M, N, K, None if ws < 0 else ws), got


def test_the_slices_tile_k(plans):
    for (M, N, K, ws), got in plans.items():
        S, kslice = got["S"], got["kslice"]
        assert 1 <= S <= 32 and kslice % 32 == 0 and (S - 1) * kslice < K <= S * kslice, got      # no slice is empty
        assert S == 1 or (ws >= S * M * N and kslice >= 128), got                               # the slabs fit the workspace


def test_the_wrapper_states_the_same_workspace(plans):
    from unidisc_amd import kernels as Kn

    for (M, N, K, ws), got in plans.items():
        assert got["need"] == Kn.skinny_ws_elems(M, N, K), got
        if ws >= got["need"] > 0:
            assert got["S"] > 1, got


def test_the_plan_does_not_depend_on_the_rows_given_the_workspace(plans):
    from unidisc_amd import kernels as Kn

    for N, K in SHAPES:
        seen = set()
        for M in ROWS:
            need = Kn.skinny_ws_elems(M, N, K)
            for ws in (need, need + 1, 40 * M * N):
                if ws >= need:
                    seen.add((plans[(M, N, K, ws)]["S"], plans[(M, N, K, ws)]["kslice"]))
        assert len(seen) == 1, (N, K, seen)
    # the engine sizes its workspace for all Bp rows: the halves of a 128-row step see the plan of a 64-row step with its own workspace
    for N, K in SHAPES:
        whole, half = plans[(128, N, K, Kn.skinny_ws_elems(128, N, K))], plans[(64, N, K, Kn.skinny_ws_elems(64, N, K))]
        assert (whole["S"], whole["kslice"]) == (half["S"], half["kslice"])


def test_the_entry_point_uses_the_header():
    src = open(os.path.join(ROOT, "unidisc_amd", "csrc", "decode.hip")).read()
    assert src.count("skinny_plan(M, N, K, ws != nullptr, ws_elems)") == 1 and '#include "skinny_plan.h"' in src
