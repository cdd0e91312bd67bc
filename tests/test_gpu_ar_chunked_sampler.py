"""eval.ar_chunk_given: the AR sampler feeds runs of columns that are given in every row through one chunk forward over the KV cache (DIT._forward_chunk)
instead of one decode step per token.

The conditioning: the text prefix, two image runs given in all rows (the second reaches the last column) and one run given in two of four rows.  With
recorded Gumbel noise the given positions equal x0, no [MASK] is left, and every generated token is the argmax of (teacher-forced logits + noise) wherever
the top-two margin exceeds 0.05 - the rule and the 90 % of tests/test_gpu_ar_sampler.py::_check_argmax_run - and equals the key-off run there; the same
under guidance.  A spy counts the calls: the partly given run takes decode steps.  The token loop makes no host synchronisation (the method of
test_sampler_has_no_host_sync_and_frees_cache).  The tensor top-p path refuses the key."""
import pytest
import torch

from test_gpu_ar_sampler import MARGIN_EPS, _ar_diff, _check_argmax_run, _excluded, _static_mod, _teacher_forced_next

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _conditioning(diff, B, seed):
    """x0, x0_unmask [B, L] and what the loop must do with them: (decode steps, chunks as (start_pos, tokens))"""
    L, Lt = diff.config.model.length, diff.config.model.txt_length
    assert (B, L, Lt) == (4, 32, 16)
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, diff.text_vocab_size - 1, (B, L), generator=gen)
    x0[:, Lt:] = torch.randint(diff.text_vocab_size, diff.vocab_size - 1, (B, L - Lt), generator=gen)      # image ids at image positions
    unmask = torch.zeros(B, L, dtype=torch.bool)
    unmask[:, :Lt] = True          # the text prefix: prefilled (n0 = 16)
    unmask[:, 18:22] = True        # given in all rows: step 17 feeds the positions 17 .. 21
    unmask[:2, 23:25] = True       # given in two of four rows: decode steps
    unmask[:, 26:32] = True        # given in all rows up to the last column: step 25 feeds the positions 25 .. 30
    return x0.to(DEV), unmask.to(DEV), [16, 22, 23, 24], [(17, 5), (25, 6)]


def _noise(B, L, V, seed):
    gen = torch.Generator().manual_seed(seed)
    return -torch.log(-torch.log(torch.rand(B, L - 1, V, generator=gen).clamp(1e-10, 1 - 1e-7))).to(DEV)


def _spy(bb):
    calls = dict(decode=[], chunk=[])
    dec, chk = bb._decode_step, bb._forward_chunk

    def decode(p):
        calls["decode"].append(p)
        return dec(p)

    def chunk(ids, modality, p, last_only=False):
        assert last_only
        calls["chunk"].append((p, ids.shape[1]))
        return chk(ids, modality, p, last_only=last_only)

    bb._decode_step, bb._forward_chunk = decode, chunk
    return calls


def _sure(diff, x, noise, mod, z_of):
    z = (z_of(x)[:, :-1] + noise).masked_fill(_excluded(diff, mod[:, 1:]), float("-inf"))
    top2 = z.topk(2, -1).values
    return (top2[..., 0] - top2[..., 1]) > MARGIN_EPS


@pytest.mark.parametrize("guided", [False, True])
def test_chunked_sampler_replays_noise_and_equals_the_decode_path(guided):
    diff = _ar_diff(6)
    if guided:
        diff.config.eval.cfg = 1.5
        diff.config.eval.force_cfg_value = True
    B, L, V = 4, diff.config.model.length, diff.vocab_size
    mod = _static_mod(diff, B)
    x0, unmask, decode_steps, chunks = _conditioning(diff, B, 21)
    noise = _noise(B, L, V, 13)
    x_off, nfe_off = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, noise=noise, bos_token_id=3)
    diff.config.eval.ar_chunk_given = True
    diff.config.eval.ar_chunk_min_tokens = 2
    calls = _spy(diff.backbone)
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, noise=noise, bos_token_id=3)
    assert calls == dict(decode=decode_steps, chunk=chunks)
    assert nfe == nfe_off == L - 1
    assert torch.equal(x[unmask], x0[unmask]) and not (x == diff.mask_index).any()

    def z_of(xx):
        if not guided:
            return _teacher_forced_next(diff, xx, mod)
        xu = torch.where(unmask, diff.mask_index, xx)
        return 2.5 * _teacher_forced_next(diff, xx, mod) - 1.5 * _teacher_forced_next(diff, xu, mod)

    _check_argmax_run(diff, x, nfe, noise, mod, z_of, x0, unmask)
    _check_argmax_run(diff, x_off, nfe_off, noise, mod, z_of, x0, unmask)
    # the key-off run: equal wherever the margin is sure (in both runs' own teacher-forced rows) and the row's earlier tokens agree - a near tie the two
    # paths' bf16 logits order differently changes what the row is conditioned on from there
    sure = _sure(diff, x, noise, mod, z_of) & _sure(diff, x_off, noise, mod, z_of)

    def same_where_sure(xa):
        eq = xa[:, 1:] == x_off[:, 1:]
        earlier = torch.cat([torch.ones_like(eq[:, :1]), eq[:, :-1].long().cumprod(1).bool()], 1)
        return bool(eq[sure & earlier].all())

    assert same_where_sure(x), "a sure position differs between the chunked and the decode-path run"
    # a longer minimum leaves the first run (5 tokens) on the decode path
    diff.config.eval.ar_chunk_min_tokens = 6
    calls["decode"].clear(), calls["chunk"].clear()
    x6, _ = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, noise=noise, bos_token_id=3)
    assert calls == dict(decode=list(range(16, 25)), chunk=[(25, 6)])
    assert same_where_sure(x6)


def test_key_unset_takes_decode_steps_only():
    diff = _ar_diff(6)
    B = 4
    mod = _static_mod(diff, B)
    x0, unmask, _, _ = _conditioning(diff, B, 21)
    calls = _spy(diff.backbone)
    diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, seed=3, bos_token_id=3)
    assert calls == dict(decode=list(range(16, 31)), chunk=[])


def test_chunked_sampler_has_no_host_sync_in_the_loop():
    """Diffusion._ar_sampler with the key under torch.cuda.set_sync_debug_mode("error"); the two host reads of the run - the prefix length and the columns
    given in every row, both before the token loop - are taken outside (the same values), so that the rest of the run, the loop included, is checked."""
    diff = _ar_diff(4)
    diff.config.eval.ar_chunk_given = True
    diff.config.eval.ar_chunk_min_tokens = 2
    B, L = 4, diff.config.model.length
    mod = _static_mod(diff, B)
    x0, unmask, decode_steps, chunks = _conditioning(diff, B, 4)
    n0, given = type(diff)._ar_fixed_prefix(unmask, L), type(diff)._ar_given_columns(unmask)
    diff._ar_fixed_prefix = lambda u, LL: n0
    diff._ar_given_columns = lambda u: given
    diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, seed=9, bos_token_id=3)   # (warm-up: first launches, allocator)
    torch.cuda.synchronize()
    calls = _spy(diff.backbone)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, seed=9, bos_token_id=3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert calls == dict(decode=decode_steps, chunk=chunks)
    assert nfe == L - 1 and not (x[:, 1:] == diff.mask_index).any() and torch.equal(x[unmask], x0[unmask])
    assert diff.backbone._kv is None


def test_tensor_top_p_refuses_the_key():
    diff = _ar_diff(3)
    diff.config.eval.top_p = 0.8
    diff.config.eval.ar_chunk_given = True
    B = 4
    mod = _static_mod(diff, B)
    x0, unmask, _, _ = _conditioning(diff, B, 5)
    with pytest.raises(NotImplementedError, match="ar_chunk_given"):
        diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, seed=5, bos_token_id=3)
    assert diff.backbone._kv is None
    diff.config.eval.ar_chunk_given = False
    x, nfe = diff._ar_sampler(B, x0=x0, x0_unmask=unmask, modality=mod, seed=5, bos_token_id=3)      # the same configuration without the key runs
    assert nfe == 0 and torch.equal(x[unmask], x0[unmask])
