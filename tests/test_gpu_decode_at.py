"""The decode step's device-position entry points on a real MI355X (pytest -m gpu), eagerly - no graph here: udm_attention_decode_at,
udm_ar_sample_rows_at, udm_ar_nucleus_rows_at, udm_decode_stage and udm_counter_add read the position from device memory and must leave bit for bit
what the host-position calls leave.

Attention: both forms run on clones of one arena - guard | K cache | guard | V cache | guard, bf16, the guards four cache slots long (so at least one
slot lies behind slot Lmax - 1 of the last row), every slot from p upwards NaN, the split workspace NaN too (a partial read that this position did not
write would poison o) - and the WHOLE arena, o and nothing else are compared: slot p, every other cache byte and the guards.  Lmax = 200, B H up to
192 (ceil(512 / B H) = 3: S(190) = 3 but S(200) = 2, the grid is sized by the bound), p on both sides of every 64-key boundary.  A position outside
[0, Lmax) (and outside x for the token choice) stores nothing: arena and outputs keep every bit.  Each kernel returns on such a position before its
first access, so those calls touch no memory at all."""
import pytest
import torch

from unidisc_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
LMAX = 200
POSITIONS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 189, 199]
GUARD_SLOTS = 4


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF16 else (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t)


def _pos(p):
    return torch.tensor([p], dtype=torch.int64, device=DEV)


def _base(B, H, D, gen):
    """random K and V caches [B, Lmax, d], made once per test: every position's arena takes its slots below p from them"""
    return [torch.randn((B, LMAX, H * D), generator=gen).to(DEV).to(BF16) for _ in range(2)]


def _arena(B, H, D, p, base):
    """(arena, K view, V view): slots [0, p) random, [p, Lmax) NaN, guards a finite pattern"""
    d = H * D
    n = B * LMAX * d
    g = GUARD_SLOTS * d
    arena = torch.full((3 * g + 2 * n,), 7.0, dtype=BF16, device=DEV)
    Kc = arena[g:g + n].view(B, LMAX, d)
    Vc = arena[2 * g + n:2 * g + 2 * n].view(B, LMAX, d)
    for c, src in zip((Kc, Vc), base):
        c[:, :p] = src[:, :p]
        c[:, p:] = float("nan")
    return arena, Kc, Vc


def _operands(B, H, D, padded, gen):
    """q, k_new, v_new and the row stride of o: the engine's views (columns of the [Bp, 2d] qk-norm output and the [Bp, 3d] qkv), or padded rows"""
    d = H * D
    if padded:
        bufs = [torch.randn((B, d + 8 * (i + 1)), generator=gen).to(DEV).to(BF16) for i in range(3)]
        return bufs[0][:, :d], bufs[1][:, :d], bufs[2][:, :d], d + 32
    qkr = torch.randn((B, 2 * d), generator=gen).to(DEV).to(BF16)
    qkv = torch.randn((B, 3 * d), generator=gen).to(DEV).to(BF16)
    return qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], d


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("B,H", [(1, 2), (8, 2), (8, 24)])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_attention_decode_at_equals_the_host_position_call(D, B, H, padded):
    gen = torch.Generator().manual_seed(D + 7 * B + H)
    d = H * D
    q, kn, vn, ldo = _operands(B, H, D, padded, gen)
    base = _base(B, H, D, gen)
    for p in POSITIONS:
        arena, Kc, Vc = _arena(B, H, D, p, base)
        arena2 = arena.clone()
        g, n = GUARD_SLOTS * d, B * LMAX * d
        Kc2, Vc2 = arena2[g:g + n].view(B, LMAX, d), arena2[2 * g + n:2 * g + 2 * n].view(B, LMAX, d)
        ws = [K.attention_decode_ws(B, H, D, DEV).fill_(float("nan")) for _ in range(2)]
        o = [torch.full((B, ldo), -3.0, dtype=BF16, device=DEV) for _ in range(2)]
        K.attention_decode(q, kn, vn, Kc, Vc, p, H, D, out=o[0][:, :d], ws=ws[0])
        K.attention_decode_at(q, kn, vn, Kc2, Vc2, _pos(p), H, D, out=o[1][:, :d], ws=ws[1])
        torch.cuda.synchronize()
        assert torch.isfinite(o[0][:, :d].float()).all(), p
        assert torch.equal(_bits(o[0]), _bits(o[1])), p                               # o, and the padding of its rows
        assert torch.equal(_bits(Kc[:, p]), _bits(kn)) and torch.equal(_bits(Vc2[:, p]), _bits(vn)), p
        assert torch.equal(_bits(arena), _bits(arena2)), p                           # slot p, every other slot, the guards
        want = K.attention_decode_s_bound(B * H, LMAX)
        assert want == (3 if B * H == 192 else 4)


@pytest.mark.parametrize("B,H,D", [(1, 2, 32), (8, 24, 128), (8, 2, 256)])
@pytest.mark.parametrize("p", [-1, LMAX, LMAX + 63, 1 << 40, -(1 << 40)])
def test_attention_decode_at_out_of_range_stores_nothing(B, H, D, p):
    gen = torch.Generator().manual_seed(3)
    d = H * D
    q, kn, vn, ldo = _operands(B, H, D, False, gen)
    arena, Kc, Vc = _arena(B, H, D, 70, _base(B, H, D, gen))
    before = arena.clone()
    ws = K.attention_decode_ws(B, H, D, DEV).fill_(float("nan"))
    o = torch.full((B, ldo), -3.0, dtype=BF16, device=DEV)
    K.attention_decode_at(q, kn, vn, Kc, Vc, _pos(p), H, D, out=o, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena), _bits(before)) and (o == -3.0).all() and torch.isnan(ws).all()


def test_attention_decode_at_without_workspace_is_one_split():
    gen = torch.Generator().manual_seed(5)
    B, H, D, p = 8, 2, 64, 150
    q, kn, vn, _ = _operands(B, H, D, False, gen)
    arena, Kc, Vc = _arena(B, H, D, p, _base(B, H, D, gen))
    arena2 = arena.clone()
    g, n = GUARD_SLOTS * H * D, B * LMAX * H * D
    Kc2, Vc2 = arena2[g:g + n].view(B, LMAX, H * D), arena2[2 * g + n:2 * g + 2 * n].view(B, LMAX, H * D)
    o0 = K.attention_decode(q, kn, vn, Kc, Vc, p, H, D)
    o1 = K.attention_decode_at(q, kn, vn, Kc2, Vc2, _pos(p), H, D)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o0), _bits(o1)) and torch.equal(_bits(arena), _bits(arena2))


# ------------------------------------------------------------------------------------------------ token choice
V, VT, LD, LX, MASK = 1000, 600, 1000, 12, 999


def _choice_case(R, guided, gen):
    rows = 2 * R if guided else R
    logits = (torch.randn((rows, LD), generator=gen) * 3).to(DEV).to(BF16)
    mod = torch.randint(0, 2, (R, LX), generator=gen).to(DEV)
    x0 = torch.randint(0, V - 1, (R, LX), generator=gen).to(DEV)
    unmask = (torch.rand((R, LX), generator=gen) < 0.3).to(DEV)
    w = torch.full((4,), 1.5, dtype=torch.float32, device=DEV)
    return logits, mod, x0, unmask, w


def _state(R):
    return torch.full((R, LX), -5, dtype=torch.int64, device=DEV), torch.full((2 * R + 2,), -9, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("kind", ["gumbel", "nucleus"])
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_token_choice_at_equals_the_host_position_call(R, guided, explicit, kind):
    gen = torch.Generator().manual_seed(17 * R + 2 * guided + explicit)
    logits, mod, x0, unmask, w = _choice_case(R, guided, gen)
    noise = torch.rand((R, (LX - 1) * V), generator=gen).clamp(1e-6, 1 - 1e-6).to(DEV)
    if kind == "gumbel":
        noise = -torch.log(-torch.log(noise))
    kw = dict(modality=mod, restrict=True, seed=1234, x0=x0, x0_unmask=unmask, logits_u=logits[R:] if guided else None, w=w if guided else None, rows=R)
    for i in (0, 5, LX - 2):
        (xa, na), (xb, nb) = _state(R), _state(R)
        if kind == "gumbel":
            K.ar_sample_rows(logits, xa, i + 1, V, VT, MASK, step=i, g=noise if explicit else None, g_col0=i * V, next_ids=na, **kw)
            K.ar_sample_rows_at(logits, xb, _pos(i), V, VT, MASK, g=noise if explicit else None, next_ids=nb, **kw)
        else:
            K.ar_nucleus_rows(logits, xa, i + 1, V, VT, MASK, inv_temperature=1 / 0.7, budget=0.8, step=i, u=noise if explicit else None, u_col0=i * V,
                              next_ids=na, **kw)
            K.ar_nucleus_rows_at(logits, xb, _pos(i), V, VT, MASK, inv_temperature=1 / 0.7, budget=0.8, u=noise if explicit else None, next_ids=nb, **kw)
        torch.cuda.synchronize()
        assert (xa[:, i + 1] >= 0).all() and (na[:R] >= 0).all() and (na[2 * R:] == -9).all()
        assert (xa[:, :i + 1] == -5).all() and (xa[:, i + 2:] == -5).all()
        assert torch.equal(xa, xb) and torch.equal(na, nb), i


@pytest.mark.parametrize("kind", ["gumbel", "nucleus"])
@pytest.mark.parametrize("i", [-1, LX - 1, LX, 1 << 40])
def test_token_choice_at_out_of_range_stores_nothing(i, kind):
    R = 3
    gen = torch.Generator().manual_seed(23)
    logits, mod, x0, unmask, w = _choice_case(R, True, gen)
    noise = torch.rand((R, (LX - 1) * V), generator=gen).clamp(1e-6, 1 - 1e-6).to(DEV)
    x, nxt = _state(R)
    kw = dict(modality=mod, restrict=True, seed=1, x0=x0, x0_unmask=unmask, logits_u=logits[R:], w=w, rows=R, next_ids=nxt)
    if kind == "gumbel":
        K.ar_sample_rows_at(logits, x, _pos(i), V, VT, MASK, g=noise, **kw)
    else:
        K.ar_nucleus_rows_at(logits, x, _pos(i), V, VT, MASK, inv_temperature=1.0, budget=0.9, u=noise, **kw)
    torch.cuda.synchronize()
    assert (x == -5).all() and (nxt == -9).all()


# ------------------------------------------------------------------------------------------------ staged operands, the counter
@pytest.mark.parametrize("per_sample", [False, True])
def test_decode_stage_copies_the_positions_rows(per_sample):
    gen = torch.Generator().manual_seed(31)
    L, Bp, half = 37, 8, 16
    mod_cols = torch.randint(0, 2, (L, Bp), generator=gen).to(DEV)
    shape = (L, Bp, half) if per_sample else (L, half)
    cos, sin = torch.randn(shape, generator=gen).to(DEV), torch.randn(shape, generator=gen).to(DEV)
    for p in (0, 7, L - 1, -1, L, 1 << 40):
        mod_row = torch.full((Bp,), -4, dtype=torch.int64, device=DEV)
        cos_row, sin_row = torch.full_like(cos[:1], -2.0), torch.full_like(sin[:1], -2.0)
        K.decode_stage(_pos(p), mod_cols=mod_cols, mod_row=mod_row, cos=cos, sin=sin, cos_row=cos_row, sin_row=sin_row)
        torch.cuda.synchronize()
        if 0 <= p < L:
            assert torch.equal(mod_row, mod_cols[p]) and torch.equal(cos_row, cos[p][None]) and torch.equal(sin_row, sin[p][None]), p
        else:
            assert (mod_row == -4).all() and (cos_row == -2.0).all() and (sin_row == -2.0).all(), p
    # the rotary rows alone (no modality embedding), and the modality column alone
    cos_row = torch.zeros_like(cos[:1])
    sin_row = torch.zeros_like(sin[:1])
    K.decode_stage(_pos(5), cos=cos, sin=sin, cos_row=cos_row, sin_row=sin_row)
    mod_row = torch.zeros(Bp, dtype=torch.int64, device=DEV)
    K.decode_stage(_pos(6), mod_cols=mod_cols, mod_row=mod_row)
    torch.cuda.synchronize()
    assert torch.equal(cos_row, cos[5][None]) and torch.equal(sin_row, sin[5][None]) and torch.equal(mod_row, mod_cols[6])


def test_counter_add():
    c = torch.tensor([41, 77], dtype=torch.int64, device=DEV)
    for delta, want in ((1, 42), (5, 47), (-48, -1), (1 << 40, (1 << 40) - 1)):
        K.counter_add(c[:1], delta)
        torch.cuda.synchronize()
        assert c.tolist() == [want, 77]
