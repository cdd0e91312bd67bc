"""Where a workgroup of udm_attention_fwd_kv_causal stops walking key tiles: attn_kv_causal_walk_end of unidisc_amd/csrc/attention_plan.h, compiled alone with
a host compiler (tests/attention_kv_causal_plan_print.cpp) and compared with brute force over the mask for every 1 <= Lq <= Lk <= 320 and every 128-query
tile.  The mask is the one of tests/attention_ref64.py: query i sees key j iff j <= i + (Lk - Lq).  Required of the walk [0, end): every key a live query of
the tile sees lies in a walked 64-key tile, the last walked tile holds such a key (no tile is walked for nothing), and end never passes ceil(Lk / 64)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_L = 320
EXTRA = ((77, 333), (48, 560), (256, 512), (256, 1280))      # shapes past the sweep: two of the GPU case list, two chunk shapes of the AR sampler


@pytest.fixture(scope="module")
def ends(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++)"
    exe = str(tmp_path_factory.mktemp("attention_kv_causal_plan") / "attention_kv_causal_plan_print")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "unidisc_amd", "csrc"),
           os.path.join(ROOT, "tests", "attention_kv_causal_plan_print.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe, str(MAX_L)] + [str(x) for pair in EXTRA for x in pair], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    out = {}
    for ln in run.stdout.splitlines():
        Lq, Lk, t, end = map(int, ln.split())
        out[(Lq, Lk, t)] = end
    return out


def _brute(Lq, Lk, t):
    """the last key any live query of tile t sees: row i sees the keys {j < Lk : j <= i + (Lk - Lq)}, row by row"""
    rows = np.arange(128 * t, min(128 * t + 128, Lq))
    return int(np.minimum(rows + (Lk - Lq), Lk - 1).max())


def test_every_tile_was_printed(ends):
    assert len(ends) == sum((Lq + 127) // 128 for Lk in range(1, MAX_L + 1) for Lq in range(1, Lk + 1)) + sum((Lq + 127) // 128 for Lq, _ in EXTRA)


def test_walk_end_against_brute_force(ends):
    bad = []
    for (Lq, Lk, t), end in ends.items():
        last = _brute(Lq, Lk, t)                      # keys [0, last] are visible to the tile's last live query, nothing behind it to any
        if not (last < 64 * end and last >= 64 * (end - 1) and 1 <= end <= (Lk + 63) // 64):
            bad.append((Lq, Lk, t, end, last))
    assert not bad, bad[:10]


def test_written_out_cases(ends):
    """the case list of tests/attention_kv_causal_cases.py and the chunk shapes of the AR sampler, by hand"""
    expect = {(1, 1, 0): 1, (1, 200, 0): 4, (5, 5, 0): 1, (64, 128, 0): 2, (77, 333, 0): 6, (129, 193, 0): 3, (129, 193, 1): 4, (130, 130, 0): 2,
              (130, 130, 1): 3, (200, 264, 0): 3, (200, 264, 1): 5, (64, 320, 0): 5, (128, 320, 0): 5, (256, 320, 0): 3, (256, 320, 1): 5, (48, 560, 0): 9, (256, 512, 0): 6, (256, 512, 1): 8,
              (256, 1280, 0): 18, (256, 1280, 1): 20}
    assert {k: ends[k] for k in expect} == expect
