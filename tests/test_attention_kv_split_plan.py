"""The key-split plan of udm_attention_fwd_kv_split: attn_plan_fwd_kv_split / attn_kv_split_clamp / attn_kv_split_range of unidisc_amd/csrc/attention_plan.h,
compiled alone with a host compiler (tests/attention_kv_split_plan_print.cpp).  For every shape tests/test_gpu_attention_kv_split.py calls and for the
conditional-sampling shapes of the 1.4 B, UniDisc-S and xxl models: the split count, the grid, the per-split key-tile ranges and the workspace size.
Properties on every case: every split is non-empty, the ranges tile [0, ceil(Lk / 64)) exactly and are balanced, S = 1 wherever the unsplit grid already fills
half of the workgroup slots (2 per CU at head dim <= 128, 1 at 256) - the rule as measured is stricter: S = 1 from a quarter of the slots on, otherwise the smallest
power of two that brings the grid to half of the slots, with two key tiles left per split (RESULTS.md "Conditioning K/V cache").  Expected numbers of the named cases are written out, not computed from the header."""
import os
import shutil
import subprocess

import pytest

import attention_kv_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
WGS = {32: 2, 64: 2, 128: 2, 256: 1}

CASES = {}   # name -> ("D B H Lq Lk cus splits ws", problem dict)


def case(name, B, H, Lq, Lk, D, splits=0, ws=-1, cus=CUS):
    assert name not in CASES
    CASES[name] = (f"{D} {B} {H} {Lq} {Lk} {cus} {splits} {ws}", dict(B=B, H=H, Lq=Lq, Lk=Lk, D=D, splits=splits, ws=ws, cus=cus))


# ---- tests/test_gpu_attention_kv_split.py: B = 1 and 2, H = 2, every shape x head dim x (forced 2, 3, 8; auto)
for Lq, Lk in C.SHAPES:
    for D in C.HEAD_DIMS:
        for B in (1, 2):
            for S in (0, 2, 3, 8):
                case(f"rowwise_{B}x2x{Lq}x{Lk}x{D}_s{S}", B, 2, Lq, Lk, D, splits=S)
# ---- conditional sampling (DESIGN.md "Conditioning K/V cache"): generated slice x full length, unguided (B = 1, 8) and guided (2 B rows)
case("1p4b_caption_B1", 1, 16, 256, 1280, 128)
case("1p4b_caption_B1_cfg", 2, 16, 256, 1280, 128)
case("1p4b_caption_B8", 8, 16, 256, 1280, 128)
case("1p4b_t2i_B1", 1, 16, 1024, 1280, 128)
case("1p4b_t2i_B1_cfg", 2, 16, 1024, 1280, 128)
case("1p4b_t2i_B8", 8, 16, 1024, 1280, 128)
case("small_caption_B1", 1, 12, 128, 384, 64)
case("small_t2i_B1", 1, 12, 256, 384, 64)
case("small_t2i_B64", 64, 12, 256, 384, 64)
case("xxl_caption_B1", 1, 16, 256, 1280, 256)
case("xxl_t2i_B1", 1, 16, 1024, 1280, 256)
# ---- the lowering of a request: above the tile count, above 32, a workspace that holds fewer, no workspace
case("lower_tiles", 1, 2, 8, 72, 64, splits=8)                       # 2 key tiles
case("lower_32", 1, 2, 8, 64 * 40, 32, splits=40)
case("lower_ws_2", 1, 2, 48, 560, 64, splits=8, ws=2 * 2 * 48 * 66 + 5)   # room for 2 splits and a few floats
case("lower_ws_0", 1, 2, 48, 560, 64, splits=8, ws=2 * 48 * 66)           # room for one split's partials: no split
case("lower_null", 1, 2, 48, 560, 64, splits=8, ws=-2)
case("nine_in_four", 1, 2, 48, 560, 64, splits=4)

EXPECT = {   # name -> (S, ranges)
    "1p4b_caption_B1": (8, "0-3,3-6,6-9,9-12,12-14,14-16,16-18,18-20"),
    "1p4b_caption_B1_cfg": (4, "0-5,5-10,10-15,15-20"),
    "1p4b_caption_B8": (1, "0-20"),
    "1p4b_t2i_B1": (1, "0-20"),                                  # 128 workgroups, a quarter of the slots: split measured slower
    "1p4b_t2i_B1_cfg": (1, "0-20"),
    "1p4b_t2i_B8": (1, "0-20"),
    "small_caption_B1": (2, "0-3,3-6"),
    "small_t2i_B1": (2, "0-3,3-6"),
    "small_t2i_B64": (1, "0-6"),
    "xxl_caption_B1": (4, "0-5,5-10,10-15,15-20"),
    "xxl_t2i_B1": (1, "0-20"),
    "lower_tiles": (2, "0-1,1-2"),
    "lower_32": (32, None),
    "lower_ws_2": (2, "0-5,5-9"),
    "lower_ws_0": (1, "0-9"),
    "lower_null": (1, "0-9"),
    "nine_in_four": (4, "0-3,3-5,5-7,7-9"),
    "rowwise_2x2x48x560x64_s0": (4, "0-3,3-5,5-7,7-9"),       # 4 workgroups unsplit; 9 tiles: 32 -> 4 keeps two tiles per split
    "rowwise_1x2x8x72x128_s0": (1, "0-2"),                    # two key tiles: nothing to split
    "rowwise_1x2x77x333x32_s3": (3, "0-2,2-4,4-6"),
    "rowwise_2x2x128x640x256_s8": (8, "0-2,2-4,4-5,5-6,6-7,7-8,8-9,9-10"),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("attention_kv_split_plan") / "attention_kv_split_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"),
           os.path.join(ROOT, "tests", "attention_kv_split_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], input="".join(f"{line} {name}\n" for name, (line, _) in CASES.items()), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        name, *fields = ln.split()
        out[name] = dict(f.split("=") for f in fields)
    return out


def test_every_case_was_planned(plans):
    assert set(plans) == set(CASES) and set(EXPECT) <= set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_split_plan_properties(plans, name):
    p, prob = plans[name], CASES[name][1]
    S, T = int(p["S"]), -(-prob["Lk"] // 64)
    unsplit = -(-prob["Lq"] // 128) * prob["B"] * prob["H"]
    assert int(p["kv_tiles"]) == T and int(p["unsplit_grid"]) == unsplit and int(p["grid_ok"]) == 1
    assert 1 <= S <= min(T, 32) and int(p["grid"]) == unsplit * S
    assert int(p["ws"]) == (0 if S == 1 else S * prob["B"] * prob["H"] * prob["Lq"] * (prob["D"] + 2))
    ranges = [tuple(int(x) for x in r.split("-")) for r in p["ranges"].split(",")]
    assert len(ranges) == S and ranges[0][0] == 0 and ranges[-1][1] == T                      # the last range carries the Lk tail
    assert all(e > b for b, e in ranges), "an empty split"
    assert all(ranges[i][1] == ranges[i + 1][0] for i in range(S - 1)), "the ranges do not tile the key tiles"
    sizes = [e - b for b, e in ranges]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)              # balanced, the longer ranges first
    auto = int(p["auto"])
    slots = prob["cus"] * WGS[prob["D"]]
    if 2 * unsplit >= slots:
        assert auto == 1, "the unsplit grid fills half of the slots: no split"
    if 4 * unsplit >= slots:
        assert auto == 1, "the unsplit grid fills a quarter of the slots: the split measured slower"
    else:
        assert auto & (auto - 1) == 0 and (auto == 1 or T // auto >= 2) and auto <= 32        # a power of two, two key tiles per split
        assert auto == 1 or 2 * unsplit * (auto // 2) < slots, "not the smallest power of two that reaches half of the slots"
        bigger = 2 * auto
        assert 2 * unsplit * auto >= slots or bigger > 32 or T // bigger < 2, "a larger split count would still be under half of the slots and keep two tiles"
    if prob["splits"] == 0:
        assert S == auto
    else:
        assert S <= prob["splits"]
        if prob["ws"] == -1:
            assert S == min(prob["splits"], T, 32)
    if prob["ws"] == -2:
        assert S == 1
    elif prob["ws"] >= 0:
        assert int(p["ws"]) <= prob["ws"]


@pytest.mark.parametrize("name", list(EXPECT))
def test_split_plan_numbers(plans, name):
    S, ranges = EXPECT[name]
    assert int(plans[name]["S"]) == S, plans[name]
    if ranges is not None:
        assert plans[name]["ranges"] == ranges, plans[name]
