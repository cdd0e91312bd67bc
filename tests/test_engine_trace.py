"""The structure of what the engine (unidisc_amd/dit.py) asks of the kernels, pinned: per case of scripts/trace_engine.py's `pin` matrix - one per mode, plus
activation checkpointing and the compacted head - the number of `K.*` calls and one hash over the call list's names, dtypes, shapes, strides, scalars and buffer
numbering (which buffer is passed where).  No data digests: those differ between machines and thread counts.  The fixture tests/golden/engine_trace.json was
written by `python scripts/trace_engine.py --matrix pin --structure tests/golden/engine_trace.json --dit <dit.py of the commit before the engine got its
records>`; a change of the engine that is meant to launch other kernels, or the same ones on other operands, regenerates it with the same command."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))

import trace_engine  # noqa: E402

with open(os.path.join(HERE, "golden", "engine_trace.json")) as f:
    PINNED = json.load(f)


@pytest.fixture(scope="module")
def traced():
    from unidisc_amd import diffusion as diff_mod, dit as dit_mod
    k_dit, k_diff = dit_mod.K, diff_mod.K
    try:
        r = trace_engine.Runner(None, "cpu")
        trace_engine.pin_matrix(r)
        return trace_engine.structure_of(r.results)
    finally:
        dit_mod.K, diff_mod.K = k_dit, k_diff


def test_the_pin_matrix_is_the_fixture_s(traced):
    assert sorted(traced) == sorted(PINNED)


@pytest.mark.parametrize("cid", sorted(PINNED))
def test_engine_makes_the_pinned_calls(cid, traced):
    assert traced[cid] == PINNED[cid], cid
