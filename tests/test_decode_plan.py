"""How the decode attention splits its keys over workgroups: unidisc_amd/csrc/decode_plan.h, compiled alone with a host compiler
(tests/decode_plan_print.cpp) and asked for the plan of every n = 1 .. 4200 at each (B H, cap).  The expected plan is the restatement below of what
udm_attention_decode computed inline before the header existed; the static bound S_bound is written out from its definition, and that it bounds S(n)
for every n <= Lmax is checked for every Lmax of the sweep - S(Lmax) itself does not (S is not monotone in n)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 4200
BHS = [1, 8, 16, 192, 256, 1024]
CAPS = [1, 2, 3, 32]


def expected(n, BH, cap):
    """(S, chunk): about two workgroups per CU over B H, at most 32 splits, at least 64 keys each, bounded by the workspace; chunk a multiple of 64"""
    S = (512 + BH - 1) // BH
    S = min(S, 32)
    S = min(S, (n + 63) // 64)
    if S > cap:
        S = cap
    if S < 1:
        S = 1
    chunk = ((n + S - 1) // S + 63) // 64 * 64
    return (n + chunk - 1) // chunk, chunk


def s_bound(BH, Lmax, cap):
    return max(1, min(-(-512 // BH), 32, -(-Lmax // 64), cap))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("decode_plan") / "decode_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"), os.path.join(ROOT, "tests", "decode_plan_print.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    cases = [(n, BH, cap) for BH in BHS for cap in CAPS for n in range(1, N_MAX + 1)]
    run = subprocess.run([exe], input="".join(f"{n} {BH} {cap}\n" for n, BH, cap in cases), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    out = {}
    for row in run.stdout.splitlines():
        f = {k: int(v) for k, v in (kv.split("=") for kv in row.split())}
        out[(f["n"], f["BH"], f["cap"])] = f
    assert sorted(out) == sorted(cases)
    return out


def test_the_plan_is_the_entry_points_rule(plans):
    for (n, BH, cap), got in plans.items():
        assert (got["S"], got["chunk"]) == expected(n, BH, cap), got
        assert got["bound"] == s_bound(BH, n, cap), got


def test_the_splits_tile_the_keys(plans):
    for (n, BH, cap), got in plans.items():
        S, chunk = got["S"], got["chunk"]
        assert 1 <= S <= min(32, cap) and chunk % 64 == 0 and chunk >= 64, got
        assert (S - 1) * chunk < n <= S * chunk, got      # [0, n) = S ranges of `chunk` keys, none empty; the last one holds key n - 1


def test_the_bound_holds_for_every_position_below_lmax(plans):
    for BH in BHS:
        for cap in CAPS:
            worst = 0                                     # max of S over n <= Lmax, running
            for Lmax in range(1, N_MAX + 1):
                worst = max(worst, plans[(Lmax, BH, cap)]["S"])
                assert worst <= plans[(Lmax, BH, cap)]["bound"], (BH, cap, Lmax, worst)


def test_s_is_not_monotone_in_n(plans):
    """ceil(512 / BH) = 3: 190 keys are three splits of 64, 200 keys two of 128 - a grid sized by S(Lmax = 200) would drop the third split of n = 190"""
    assert (plans[(190, 192, 32)]["S"], plans[(190, 192, 32)]["chunk"]) == (3, 64)
    assert (plans[(200, 192, 32)]["S"], plans[(200, 192, 32)]["chunk"]) == (2, 128)
    assert plans[(200, 192, 32)]["bound"] == 3 and s_bound(192, 200, 32) == 3


def test_the_wrapper_states_the_same_bound():
    from unidisc_amd import kernels as K

    for BH in BHS:
        for cap in CAPS:
            for Lmax in (1, 63, 64, 65, 200, 1279, 4200):
                assert K.attention_decode_s_bound(BH, Lmax, cap) == s_bound(BH, Lmax, cap)


def test_the_entry_points_use_the_header():
    src = open(os.path.join(ROOT, "unidisc_amd", "csrc", "decode.hip")).read()
    assert src.count("decode_plan(p + 1, BH, cap)") == 1 and "decode_plan_s_bound(BH, Lmax, cap)" in src
    assert "decode_plan(p + 1, (long)gridDim.x, (long)a.cap)" in src      # the kernels plan from the position they read
