"""CPU checks of the chunked cached forward's host side: the run segmentation of eval.ar_chunk_given (Diffusion._ar_given_runs, a pure function of the
columns given in every row, the prefilled prefix and the smallest chunk) on hand-written masks, and the order in which DIT.forward(start_pos=p) with several
tokens refuses: CPU tensors first, before anything else of the cache is read.  The kernel, the engine path and the sampler run on the GPU
(tests/test_gpu_attention_kv_causal_rowwise.py, tests/test_gpu_ar_chunked_forward.py, tests/test_gpu_ar_chunked_sampler.py)."""
import types

import pytest
import torch

from ar_utils import ar_config
from oracle.cases import CASES


def _runs(mask, min_tokens=2):
    """mask: string over the columns 0 .. L - 1, '1' = given in every row; the prefix as _ar_fixed_prefix counts it"""
    from unidisc_amd import Diffusion

    L = len(mask)
    unmask = torch.tensor([[c == "1" for c in mask]] * 2)
    n0 = Diffusion._ar_fixed_prefix(unmask, L)
    return n0, Diffusion._ar_given_runs(Diffusion._ar_given_columns(unmask), n0, L, min_tokens)


def test_runs_behind_the_prefix():
    #            0         1
    #            0123456789012345
    n0, runs = _runs("1110011100001100")
    assert n0 == 3                       # column 0 always, then the leading run 1 .. 2
    # columns 5 .. 7: step 4 feeds the positions 4 .. 7 (r = 3); columns 12 .. 13: step 11 feeds 11 .. 13 (r = 2)
    assert runs == {4: 3, 11: 2}


def test_a_run_touching_the_prefix_is_the_prefix():
    n0, runs = _runs("0111100000")
    assert n0 == 5 and runs == {}        # (column 0 is BOS or x0 whatever the mask says)
    n0, runs = _runs("1111100110")
    assert n0 == 5 and runs == {6: 2}


def test_short_runs_stay_on_the_decode_path():
    mask = "1000110001110000"            # runs of 2 (columns 4 .. 5: 3 tokens) and 3 (columns 9 .. 11: 4 tokens)
    assert _runs(mask, 2)[1] == {3: 2, 8: 3}
    assert _runs(mask, 3)[1] == {3: 2, 8: 3}
    assert _runs(mask, 4)[1] == {8: 3}   # a run shorter than min_tokens - 1 is dropped
    assert _runs(mask, 5)[1] == {}
    assert _runs("1001000", 2)[1] == {2: 1}      # one given column: a chunk of two tokens
    assert _runs("1001000", 3)[1] == {}


def test_a_column_missing_in_one_row_splits_a_run():
    from unidisc_amd import Diffusion

    unmask = torch.tensor([[c == "1" for c in "1000111111000000"]] * 3)
    unmask[1, 7] = False
    L = unmask.shape[1]
    n0 = Diffusion._ar_fixed_prefix(unmask, L)
    assert n0 == 1
    assert Diffusion._ar_given_runs(Diffusion._ar_given_columns(unmask), n0, L, 2) == {3: 3, 7: 2}      # columns 4 .. 6 and 8 .. 9
    unmask[2, 4:10] = False              # given in some rows only: the decode path
    assert Diffusion._ar_given_runs(Diffusion._ar_given_columns(unmask), n0, L, 2) == {}


def test_the_last_column_is_never_fed():
    # position L - 1 has no cache slot (the sampler feeds L - 1 positions): a run that reaches it is cut at L - 2 and choose(L - 2) writes the last column
    n0, runs = _runs("1000001111")
    assert n0 == 1 and runs == {5: 3}    # columns 6 .. 9, fed: the positions 5 .. 8
    assert _runs("1000000001")[1] == {}              # column 9 alone: nothing given is ever fed
    assert _runs("1000000001", 1)[1] == {}
    assert _runs("1000000011")[1] == {7: 1}          # columns 8 .. 9: the positions 7 .. 8
    assert _runs("1000000111")[1] == {6: 2}
    n0, runs = _runs("1111111111")
    assert n0 == 9 and runs == {}        # everything given: the prefix is capped at L - 1, nothing is left


def test_every_step_is_taken_once():
    """walking the loop of _ar_sampler over the segmentation: every position n0 .. L - 2 is fed exactly once, by a step or inside a chunk"""
    from unidisc_amd import Diffusion

    gen = torch.Generator().manual_seed(0)
    for _ in range(200):
        L = int(torch.randint(3, 40, (1,), generator=gen))
        unmask = (torch.rand(1, L, generator=gen) < 0.6).expand(2, L)
        n0 = Diffusion._ar_fixed_prefix(unmask, L)
        given = Diffusion._ar_given_columns(unmask)
        for min_tokens in (2, 3, 5):
            runs = Diffusion._ar_given_runs(given, n0, L, min_tokens)
            fed, i = [], n0
            while i < L - 1:
                r = runs.get(i, 0)
                assert r == 0 or (r + 1 >= min_tokens and all(given[c - 1] for c in range(i + 1, i + r + 1)))
                fed += list(range(i, i + r + 1))
                i += r + 1
            assert fed == list(range(n0, L - 1)) and all(n0 <= k for k in runs)


def test_cached_forward_refuses_cpu_tensors_first():
    from unidisc_amd import Diffusion

    bb = Diffusion(ar_config(CASES["b_small"]), None, "cpu").backbone
    x = torch.zeros(2, 3, dtype=torch.int64)
    bb._kv = types.SimpleNamespace(B=2, Bp=8, Lmax=31)      # (a stand-in without `pos`: the refusal reads nothing else of the cache)
    try:
        with pytest.raises(NotImplementedError, match=r"start_pos=4 with 3 tokens runs on HIP kernels; there is no CPU path"):
            bb(x, None, start_pos=4)
        with pytest.raises(NotImplementedError, match=r"start_pos=30 with 3 tokens"):      # even where a device call would be a ValueError (past the cache)
            bb(x, None, start_pos=30)
        with pytest.raises(NotImplementedError, match="attention_mask"):                   # the mask refusal still precedes it
            bb(x, None, start_pos=4, attention_mask=torch.ones(2, 3, dtype=torch.bool))
        with pytest.raises(ValueError, match="the cache holds 2"):                         # ... and the row count
            bb(torch.zeros(3, 3, dtype=torch.int64), None, start_pos=4)
    finally:
        bb._kv = None
