"""DIT.forward(indices[B, n], start_pos=p) with p > 0 and n > 1: the chunked KV-cached forward of the AR baseline (DIT._forward_chunk - the engine's forward on
the n positions, udm_attention_fwd_kv_causal over the cache).

On the goldens ar_b_small (1-D rope) and ar_c_large (2-D rope): a prefill of n0 tokens, then chunks of 3, 1 (the decode step), 7 and the rest.  Bounds are
those of tests/test_gpu_ar_sampler.py: every position against the full causal forward with rel_err < 1e-2, the whole against the imported reference's fp32
logits under floor_bound; every block's K and V cache after the chunks against the cache one whole prefill leaves (rel_err < 1e-2); the cache position
advances; a chunk that ends outside the cache or starts behind the written slots is a ValueError."""
import pytest
import torch

from ar_utils import ArGolden, build_ar_product
from golden_utils import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NLL_BOUND = 4.5e-3
N0 = 5
CHUNKS = (3, 1, 7)      # then the rest


def floor_bound(floor):
    return max(1.25 * floor + 5e-4, NLL_BOUND)


@pytest.fixture(scope="module", params=["ar_b_small", "ar_c_large"])
def run(request):
    """the golden, its product, the full causal forward, the chunked logits with the positions each call started at, and both caches"""
    g = ArGolden(request.param)
    diff = build_ar_product(g, DEV)
    bb = diff.backbone
    bb.eval()
    x, mod = g.t("fp32/input_ids").to(DEV), g.t("fp32/modality").to(DEV)
    B, L = x.shape
    with torch.no_grad():
        full = bb(x, None, modality=mod).float()
        bb.reset_kv_cache(batch_size=B, seq_len=L, dtype=torch.bfloat16, device=DEV, modality=mod)
        whole = bb(x, None, modality=mod, start_pos=0).float()
        K_whole, V_whole = [k[:B].clone() for k in bb._kv.K], [v[:B].clone() for v in bb._kv.V]
        bb.reset_kv_cache(batch_size=B, seq_len=L, dtype=torch.bfloat16, device=DEV, modality=mod)
        rows, starts, p = [bb(x[:, :N0], None, modality=mod[:, :N0], start_pos=0).float()], [0], N0
        positions = [bb._kv.pos]
        for n in CHUNKS + (L - N0 - sum(CHUNKS),):
            rows.append(bb(x[:, p:p + n], None, modality=mod[:, p:p + n], start_pos=p).float())
            starts.append(p)
            p += n
            positions.append(bb._kv.pos)
        K_chunk, V_chunk = [k[:B].clone() for k in bb._kv.K], [v[:B].clone() for v in bb._kv.V]
    assert p == L
    out = dict(g=g, bb=bb, x=x, mod=mod, full=full, whole=whole, chunked=torch.cat(rows, 1), shapes=[tuple(r.shape) for r in rows], starts=starts,
               positions=positions, K=(K_whole, K_chunk), V=(V_whole, V_chunk))
    yield out
    bb.reset_kv_cache(set_to_none=True)


def test_chunks_match_the_full_causal_forward(run):
    B, L = run["x"].shape
    V = run["full"].shape[-1]
    sizes = (N0,) + CHUNKS + (L - N0 - sum(CHUNKS),)
    assert sizes[-1] > 1 and run["shapes"] == [(B, n, V) for n in sizes]
    assert run["positions"] == [sum(sizes[:i + 1]) for i in range(len(sizes))]      # kv.pos advances with every call
    for p in range(L):
        assert rel_err(run["chunked"][:, p], run["full"][:, p]) < 1e-2, p
    assert rel_err(run["whole"], run["full"]) < 1e-2


def test_chunks_match_the_reference_logits(run):
    g = run["g"]
    truth = g.t("fp32/logits")
    bound = floor_bound(rel_err(g.t("bf16/logits"), truth))
    assert rel_err(run["full"].cpu(), truth) < bound
    assert rel_err(run["chunked"].cpu(), truth) < bound


def test_chunks_leave_the_cache_of_one_prefill(run):
    for name in ("K", "V"):
        whole, chunk = run[name]
        for i, (a, b) in enumerate(zip(whole, chunk)):
            assert bool(torch.isfinite(b.float()).all())
            assert rel_err(b.float(), a.float()) < 1e-2, (name, i)


def test_chunk_bounds_are_value_errors(run):
    bb, x, mod = run["bb"], run["x"], run["mod"]
    B, L = x.shape
    bb.reset_kv_cache(batch_size=B, seq_len=L - 2, dtype=torch.bfloat16, device=DEV, modality=mod)
    with torch.no_grad():
        bb(x[:, :4], None, modality=mod[:, :4], start_pos=0)
        assert bb._kv.pos == 4
        with pytest.raises(ValueError, match="start_pos=6"):       # slots 4 and 5 were never written
            bb(x[:, 6:9], None, modality=mod[:, 6:9], start_pos=6)
        with pytest.raises(ValueError, match=f"start_pos=4 with {L - 5} tokens"):      # ends one slot behind the cache
            bb(x[:, 4:L - 1], None, modality=mod[:, 4:L - 1], start_pos=4)
        assert bb._kv.pos == 4                                     # a refused call moves nothing
        out = bb(x[:, 4:L - 2], None, modality=mod[:, 4:L - 2], start_pos=4)      # ... and the chunk that ends exactly at the cache's end runs
        assert out.shape[1] == L - 6 and bb._kv.pos == L - 2
        again = bb(x[:, 2:5], None, modality=mod[:, 2:5], start_pos=2)             # rewriting written slots is allowed
        assert bb._kv.pos == 5 and rel_err(again.float(), run["full"][:, 2:5]) < 1e-2
