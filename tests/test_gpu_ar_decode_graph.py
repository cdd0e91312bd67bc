"""eval.ar_decode_graph on a real MI355X (pytest -m gpu): the AR sampler's decode step, token choice and position advance captured once into a graph
and replayed per token (DIT.capture_decode_step) against the same sampler with the key off.

The replayed step launches the host-position step's kernels on the same operands (tests/test_gpu_decode_at.py: bit-identical), so its logits are
bit-identical and the whole x must be EQUAL - no near-tie allowance.  model.length = 160 (96 text + 64 image positions) at the width of the tiny AR
product: the decode crosses 64 -> 65 and 128 -> 129 keys inside the replay, where the attention's split changes under the fixed grid.  1-D rope, and
2-D rope (per-row rotary rows staged from the full-length tables).  Also: the ledger, no synchronising call in the token loop, and a second sample()
in the same process (a capture per call on that call's buffers)."""
import types

import pytest
import torch

from ar_utils import ar_config
from oracle.cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, LT, LI = 4, 96, 64
L = LT + LI


def _diff(rope_2d=False, seed=0, **eval_kw):
    from unidisc_amd import Diffusion

    case = dict(CASES["c_large" if rope_2d else "b_small"], txt_length=LT, img_length=LI)
    torch.manual_seed(seed)
    diff = Diffusion(ar_config(case), None, DEV)
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "embed" in n or "attn" in n or "mlp" in n:
                p.copy_((torch.randn(p.shape, generator=gen) * 2 / p.shape[-1] ** 0.5).to(DEV))
    diff.backbone.eval()
    diff.tokenizer = types.SimpleNamespace(bos_token_id=3)      # (sample() takes the BOS id from the tokenizer)
    for k, v in eval_kw.items():
        setattr(diff.config.eval, k, v)
    assert diff.config.model.length == L and diff.backbone.rope_2d == rope_2d
    return diff


def _mod(diff):
    mod = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    mod[:, diff.static_img_sl] = 1
    return mod


def _conditioning(diff, ragged=True, run=None):
    """x0 / x0_unmask: a text prefix of another length in every row (ragged: the common prefix is the shortest), optionally a run given in all rows"""
    gen = torch.Generator().manual_seed(8)
    x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen)
    x0[:, LT:] = torch.randint(diff.text_vocab_size, diff.vocab_size - 1, (B, LI), generator=gen)
    unmask = torch.zeros(B, L, dtype=torch.bool)
    for r in range(B):
        unmask[r, :(40 + 9 * r if ragged else 40)] = True
    if run is not None:
        unmask[:, run[0]:run[1]] = True
    return x0.to(DEV), unmask.to(DEV)


def _both(diff, **kw):
    """sample() with the key off, then on: (x_off, nfe_off, stats_off, x_on, nfe_on, stats_on)"""
    diff.config.eval.ar_decode_graph = False
    x_off, nfe_off = diff.sample(return_nfe=True, **kw)
    s_off = dict(diff.ar_decode_stats)
    diff.config.eval.ar_decode_graph = True
    x_on, nfe_on = diff.sample(return_nfe=True, **kw)
    torch.cuda.synchronize()
    return x_off, nfe_off, s_off, x_on, nfe_on, dict(diff.ar_decode_stats)


def _check(out, n0, chunks=0, chunk_tokens=0):
    x_off, nfe_off, s_off, x_on, nfe_on, s_on = out
    steps = L - 1 - n0 - chunk_tokens          # decode positions n0 .. L - 2 but those inside a chunk
    assert torch.equal(x_on, x_off) and nfe_on == nfe_off
    assert s_off == dict(captures=0, replays=0, eager_steps=steps, chunks=chunks)
    assert s_on == dict(captures=1, replays=steps, eager_steps=0, chunks=chunks)


@pytest.mark.parametrize("rope_2d", [False, True])
def test_unconditional_philox(rope_2d):
    diff = _diff(rope_2d, seed=1)
    out = _both(diff, batch_size=B, modality=_mod(diff), seed=7)
    _check(out, 1)
    assert not (out[3][:, 1:] == diff.mask_index).any() and (out[3][:, LT:] >= diff.text_vocab_size).all()      # image ids at image positions


def test_recorded_noise():
    diff = _diff(seed=2)
    gen = torch.Generator().manual_seed(11)
    noise = -torch.log(-torch.log(torch.rand(B, L - 1, diff.vocab_size, generator=gen).clamp(1e-10, 1 - 1e-7))).to(DEV)
    out = _both(diff, batch_size=B, modality=_mod(diff), noise=noise)
    _check(out, 1)
    diff.config.eval.ar_decode_graph = True
    x_other = diff.sample(batch_size=B, modality=_mod(diff), noise=noise.flip(0))
    assert not torch.equal(x_other, out[3])      # (the noise is read)


@pytest.mark.parametrize("rope_2d", [False, True])
def test_conditioned_ragged_prefix(rope_2d):
    diff = _diff(rope_2d, seed=3)
    x0, unmask = _conditioning(diff)
    out = _both(diff, x0=x0, x0_unmask=unmask, modality=_mod(diff), seed=5)
    _check(out, 40)
    assert torch.equal(out[3][unmask], x0[unmask])


def test_guided():
    diff = _diff(seed=4, cfg=1.5, force_cfg_value=True)
    x0, unmask = _conditioning(diff)
    out = _both(diff, x0=x0, x0_unmask=unmask, modality=_mod(diff), seed=5)
    _check(out, 40)
    diff.config.eval.cfg = 0.0
    x_w0 = diff.sample(x0=x0, x0_unmask=unmask, modality=_mod(diff), seed=5)
    assert not torch.equal(x_w0, out[3])         # (the weight is read)


@pytest.mark.parametrize("guided", [False, True])
def test_fused_nucleus(guided):
    kw = dict(cfg=1.5, force_cfg_value=True) if guided else {}
    diff = _diff(seed=5, top_p=0.8, temperature=0.7, fused_nucleus=True, **kw)
    x0, unmask = _conditioning(diff)
    out = _both(diff, x0=x0, x0_unmask=unmask, modality=_mod(diff), seed=6)
    assert out[1] == out[4] == 0                 # (nfe with top_p: the reference's quirk)
    _check(out, 40)


def test_chunk_given_run_in_the_middle():
    diff = _diff(seed=6, ar_chunk_given=True)
    x0, unmask = _conditioning(diff, ragged=False, run=(100, 110))      # columns 100 .. 109 in every row: step 99 feeds the positions 99 .. 109
    out = _both(diff, x0=x0, x0_unmask=unmask, modality=_mod(diff), seed=5)
    _check(out, 40, chunks=1, chunk_tokens=11)
    assert torch.equal(out[3][unmask], x0[unmask])


def test_two_samples_in_one_process_and_the_cache_is_freed():
    diff = _diff(seed=7, ar_decode_graph=True)
    mod = _mod(diff)
    a = diff.sample(batch_size=B, modality=mod, seed=3)
    b = diff.sample(batch_size=B, modality=mod, seed=3)
    c = diff.sample(batch_size=B, modality=mod, seed=4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert diff.backbone._kv is None and diff.ar_decode_stats["captures"] == 1


def test_no_host_sync_in_the_token_loop():
    """torch's sync debug mode "error" from the moment the capture returns (a capture synchronises by design, once, before the loop) to the end of the
    sampler: the replays, the chunk forward and the device-side position fill behind it."""
    diff = _diff(seed=8, ar_decode_graph=True, ar_chunk_given=True)
    x0, unmask = _conditioning(diff, ragged=False, run=(100, 110))
    mod = _mod(diff)
    diff.sample(x0=x0, x0_unmask=unmask, modality=mod, seed=9)      # (warm-up: first launches, allocator)
    torch.cuda.synchronize()
    bb = diff.backbone
    capture = bb.capture_decode_step
    prev = torch.cuda.get_sync_debug_mode()

    def capture_then_watch(tail):
        g = capture(tail)
        torch.cuda.set_sync_debug_mode("error")
        return g

    bb.capture_decode_step = capture_then_watch
    try:
        x = diff.sample(x0=x0, x0_unmask=unmask, modality=mod, seed=9)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
        del bb.capture_decode_step
    torch.cuda.synchronize()
    assert diff.ar_decode_stats == dict(captures=1, replays=L - 1 - 40 - 11, eager_steps=0, chunks=1)
    assert torch.equal(x[unmask], x0[unmask]) and not (x == diff.mask_index).any()


def test_a_captured_step_does_not_outlive_its_cache():
    diff = _diff(seed=9)
    bb = diff.backbone
    bb.reset_kv_cache(batch_size=B, seq_len=L - 1, dtype=torch.bfloat16, device=DEV, modality=_mod(diff))
    bb._prefill(torch.zeros(B, 3, dtype=torch.int64, device=DEV), None, last_only=True)
    bb.set_decode_position(3)
    g = bb.capture_decode_step(None)
    g.replay()
    torch.cuda.synchronize()
    assert bb._kv.pos == 4 and int(bb._kv.pos_dev) == 4
    bb.reset_kv_cache(set_to_none=True)
    with pytest.raises(RuntimeError, match="reset"):
        g.replay()
