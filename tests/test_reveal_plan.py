"""How udm_reveal_rows is launched: unidisc_amd/csrc/reveal_plan.h, compiled alone with a host compiler (tests/reveal_plan_print.cpp) and asked for the plan of
every L in 0 .. 8193.  The expected plans are written out below, not computed from the header; the instantiations reveal.hip can launch are read from its source
and must be exactly those the plans select."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (last L of the band, threads, positions per thread): the seams the GPU test steps over (tests/test_gpu_reveal_rows.py: SEAMS)
BANDS = [(64, 64, 1), (256, 256, 1), (1024, 256, 4), (2048, 1024, 2), (4096, 1024, 4), (8192, 1024, 8)]
SEAMS = [b[0] for b in BANDS[:-1]]


def expected(L):
    if L < 1 or L > 8192:
        return None
    return next((t, v) for last, t, v in BANDS if L <= last)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("reveal_plan") / "reveal_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "reveal_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], input="".join(f"{L}\n" for L in range(0, 8194)), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {}
    for row in run.stdout.splitlines():
        f = dict(kv.split("=") for kv in row.split())
        out[int(f["L"])] = f
    assert sorted(out) == list(range(0, 8194))
    return out


def test_every_length(plans):
    for L in range(0, 8194):
        got, want = plans[L], expected(L)
        if want is None:
            assert got["ok"] == "0", got
            continue
        threads, vpt = want
        assert got["ok"] == "1" and (int(got["threads"]), int(got["vpt"])) == want, got
        assert threads * vpt >= L and threads % 64 == 0                    # every position has an owner; whole waves
        assert int(got["lds"]) == 4 * (threads * vpt + 32) and int(got["lds"]) % 16 == 0 and int(got["lds"]) <= 65536, got
        if L > 64:                                                         # no band wastes more than three quarters of its slots
            assert threads * vpt <= 4 * L, got


def test_the_seams():
    assert [expected(s) != expected(s + 1) for s in SEAMS] == [True] * len(SEAMS)
    assert expected(1280) == (1024, 2) and expected(4608) == (1024, 8) and expected(384) == (256, 4)


def test_every_instance_is_selected_and_no_other(plans):
    """the <threads, positions per thread> instantiations the entry point of reveal.hip launches are exactly those the plans select"""
    src = open(os.path.join(ROOT, "unidisc_amd", "csrc", "reveal.hip")).read()
    can = {(int(a), int(b)) for a, b in re.findall(r"launch<(\d+), (\d+)>\(a, nb, p, stream\)", src)}
    selected = {(int(p["threads"]), int(p["vpt"])) for p in plans.values() if p["ok"] == "1"}
    assert can == selected == {(t, v) for _, t, v in BANDS}, (sorted(can), sorted(selected))


def test_wrapper_gate_is_the_plans():
    from unidisc_amd import kernels as K

    class OnGpu:
        is_cuda = True

        def __init__(self, L):
            self.shape = (2, L)

        def dim(self):
            return 2

    assert K.REVEAL_L_MAX == 8192 and K.reveal_supported(OnGpu(8192)) and not K.reveal_supported(OnGpu(8193)) and K.reveal_supported(OnGpu(1))
    import torch
    assert not K.reveal_supported(torch.zeros(2, 8, dtype=torch.int64))       # a CPU tensor keeps the tensor path
