"""Head dim 256: the 8-wave forward / dQ / dK-dV of csrc/attention.hip (plain, document mask + doc_ranges, causal, dropout; dK and dV are two launches at this
head dim) and the split-key decode attention of decode.hip, row by row against dense fp64 attention.

Harness, reference, families and bounds are those of tests/test_gpu_attention_rowwise.py (NaN arenas with 256 guard rows, the `separate` and `engine` layouts,
everything outside the outputs compared bit for bit, the unchanged R.BOUNDS); tests/test_attention_ref64_d256.py shows on the CPU that the bounds are reachable
at this head dim.  Shapes are the smallest at which each D = 256 path can still go wrong."""
import pytest
import torch

import attention_ref64 as R
import test_gpu_attention_rowwise as T

pytestmark = pytest.mark.gpu
D = 256


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels as K
    return K


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,H,L", [(2, 3, 100), (1, 3, 320), (1, 8, 256)])
def test_plain_d256(K, B, H, L, family, prescaled):
    """100: ragged, less than one query block, two key tiles.  320: three query blocks with a ragged last one, five key tiles (both LDS stages), also without the
    transposing LDS reads.  256 with B H = 8: the per-XCD branch of attn_block_to_work (no generated program exists at this head dim)."""
    configs = [("", T._switches(K))]
    if L == 320:
        configs.append(("tr_read0", T._switches(K, tr=0)))
    T._case(K, "test_plain_d256", "generic", family, B, H, L, D, prescaled=prescaled, configs=configs)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("layout_name", ["contiguous", "padding"])
def test_document_mask_d256(K, layout_name, family, prescaled):
    """sample_ids + doc_ranges: tile-skipping walks and the per-element id test; rows of padding are exactly 0 in O, dQ, dK, dV and hold lse2 = +inf"""
    B, H, L = 3, 2, 320
    sid = R.doc_layouts(B, L)[layout_name]
    T._case(K, "test_document_mask_d256", f"doc_{layout_name}", family, B, H, L, D, prescaled=prescaled, sample_ids=sid, configs=[("", T._switches(K))])


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("B,H,L", [(2, 3, 200), (1, 2, 384)])
def test_causal_d256(K, B, H, L, family, prescaled):
    """UDM_ATTN_CAUSAL: the triangular walks (384: the diagonal crosses on tile seams)"""
    T._case(K, "test_causal_d256", "causal", family, B, H, L, D, prescaled=prescaled, causal=True, configs=[("", T._switches(K))])


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
def test_dropout_d256(K, family, causal, prescaled):
    """udm_attention_fwd_dropout / _bwd_dropout at p = 0.25: the keep mask does not depend on the head dim"""
    B, H, L = 2, 3, 200
    T._case(K, "test_dropout_d256", "dropout_causal" if causal else "dropout", family, B, H, L, D, prescaled=prescaled, causal=causal, p_drop=T.P_DROP,
            configs=[("", T._switches(K))])


@pytest.mark.parametrize("family", R.DECODE_FAMILIES)
@pytest.mark.parametrize("p", [65, 1000])
def test_decode_d256(K, p, family):
    """udm_attention_decode at D = 256 (32 lanes per key, 8 lane groups per block, the 256-thread combine): the body of test_decode"""
    from unidisc_amd import _lib
    from unidisc_amd.kernels import _p, _s

    DEV, BF16, F32 = T.DEV, T.BF16, T.F32
    B, H = 3, 5
    d, n = H * D, p + 1
    Lmax = p + 64
    q, k, v, _ = R.make_decode_inputs(family, B, H, n, D, seed=7 * p + D)
    ref = R.attention_ref64(q, k, v, prescaled=True)
    A, F = T.Arena(BF16), T.Arena(F32)
    for name, rows, w in (("qkr", B, 2 * d), ("qkv", B, 3 * d), ("o", B, d + 8), ("kc", B * Lmax, d), ("vc", B * Lmax, d)):
        A.add(name, rows, w)
    F.add("ws", B * H * 32, D + 2)
    a, ws = A.build(), F.build()["ws"]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, -1, d)       # [B, H, n, D] -> [B, n, H D]
    a["qkr"][:, :d].copy_(rows(q)[:, 0].to(DEV))
    a["qkr"][:, d:].copy_(rows(k)[:, p].to(DEV))
    a["qkv"][:, 2 * d:].copy_(rows(v)[:, p].to(DEV))
    kc, vc = a["kc"].view(B, Lmax, d), a["vc"].view(B, Lmax, d)
    kc[:, :p].copy_(rows(k)[:, :p].to(DEV))
    vc[:, :p].copy_(rows(v)[:, :p].to(DEV))
    o = a["o"][:, :d]
    A.snapshot(o, kc[:, p], vc[:, p])
    F.snapshot(ws)
    _lib.call("udm_attention_decode", _p(a["qkr"][:, :d]), _p(a["qkr"][:, d:]), _p(a["qkv"][:, 2 * d:]), _p(kc), _p(vc), _p(o), _p(ws), ws.numel(), B, H, D, Lmax, p,
              2 * d, 2 * d, 3 * d, d + 8, _s())
    torch.cuda.synchronize()
    faults = []
    for name, ar in (("bf16", A), ("fp32", F)):
        cnt, first = ar.stray()
        if cnt:
            faults.append(f"{cnt} {name} arena elements outside the call's outputs changed (first at flat index {first})")
    if not (torch.equal(kc[:, p].view(torch.int16), a["qkr"][:, d:].view(torch.int16)) and torch.equal(vc[:, p].view(torch.int16), a["qkv"][:, 2 * d:].view(torch.int16))):
        faults.append("cache slot p does not hold the new key / value row")
    got = dict(o=o.float().cpu().reshape(B, 1, H, D).permute(0, 2, 1, 3))
    T._judge("test_decode_d256", f"decode/{B}x{H}xD{D}/p{p}/{family}", got, ref, faults, keys=("o",))
    assert not faults, "\n".join(faults)
