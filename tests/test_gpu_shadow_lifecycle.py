"""The bf16 weight shadows across the training lifecycle on the GPU (pytest -m gpu), under the observer of tests/shadow_utils.py: after every
`refresh_weight_shadows` call - i.e. at the moment a forward fixes the weights it will read - every shadow must be, exactly, torch's bf16 cast of its fp32 master.

Model: `_PLUMB` of tests/test_gpu_fullwidth_oracle.py with two blocks (d = 256, H = 4, D = 64, L = 128, V = 1001, LayerNorm), the smallest one at which the "nn"
dgrad regime exists: B = 2 is 256 rows = one whole 256-row tile over N = in = 256, so block 0's qkv / out-proj / mlp.0 dgrads read W itself and keep NO transposed
shadow; B = 1 is 128 rows, no whole tile, and the transposed shadow comes back (and stays: `sticky_t`).  Block 1 is the last block and always keeps its transposed
shadow (`compact_last_block`).  Every test asserts these preconditions through `K.gemm_nn_ok` first and FAILS if the dispatch plan stops agreeing.

The staleness checks are exact and local; only the two-pending-backwards test (bounds: the oracle's own bf16 emulation floor, the scheme of
test_training_step_matches_oracle_at_full_width) and the side-stream cast test (the 2e-3 of test_training_steps_with_fused_adamw_match_torch_adamw_with_recast)
compare floating-point results."""
import functools

import pytest
import torch

import ledger
from oracle import unidisc_oracle as O
from oracle.cases import lumina_rope_2d
from product_utils import product_config
from shadow_utils import assert_shadows_coherent, observe_shadows
from test_gpu_fullwidth_oracle import _PLUMB, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=0.5, ema_decay=0.999)
NN = ("qkv", "out", "fc1")      # the Linears of a block whose dgrad reads W itself at 256 rows
TC = pytest.mark.parametrize("tc", [True, False], ids=["adaln", "no_adaln"])


def _case(tc, n_blocks=2):
    return dict(_PLUMB, n_blocks=n_blocks, time_conditioning=tc)


def _preconditions():
    """B = 2 (256 rows) is inside gemm_nn for every in = 256 Linear of a block, B = 1 (128 rows) is outside: without both the tests below lose their subject"""
    from unidisc_amd import kernels as K

    for out in (768, 256, 1024):
        assert K.gemm_nn_ok(256, 256, out), f"gemm_nn_ok(256, 256, {out}) is False: 256 rows are no longer the nn regime"
    assert not K.gemm_nn_ok(128, 256, 768), "gemm_nn_ok(128, 256, 768) is True: 128 rows no longer want the transposed shadow"


def _product(tc, n_blocks=2):
    from unidisc_amd import Diffusion

    _preconditions()
    torch.manual_seed(0)
    diff = Diffusion(product_config(_case(tc, n_blocks)), None, DEV)
    diff.backbone.train()
    diff.rng_device = "cpu"
    wg = torch.Generator().manual_seed(5)
    with torch.no_grad():   # non-trivial head / adaLN weights (the reference zero-initialises them)
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "adaLN_modulation" in n:
                p.copy_((torch.randn(p.shape, generator=wg) * (0.5 / p.shape[-1] ** 0.5)).to(DEV))
    return diff, diff.backbone


def _batch(B, seed):
    gen = torch.Generator().manual_seed(seed)
    Lt, Vt = _PLUMB["txt_length"], _PLUMB["text_vocab_size"]
    am = torch.ones(B, Lt, dtype=torch.bool)
    am[B - 1, Lt - 17:] = False   # ragged text: one padded row
    return dict(input_ids=torch.randint(0, Vt - 1, (B, Lt), generator=gen), attention_mask=am)


@pytest.fixture()
def forms(monkeypatch):
    """the `dgrad_form` record of every engine forward, in order"""
    from unidisc_amd.dit import DIT

    seen, orig = [], DIT._engine_forward

    def spy(self, inp, mode, save):
        out, S = orig(self, inp, mode, save)
        seen.append(dict(S.dgrad_form))
        return out, S

    monkeypatch.setattr(DIT, "_engine_forward", spy)
    return seen


def _forward(diff, B, seed):
    torch.manual_seed(seed)
    return diff.training_step(_batch(B, seed), seed)


def _eval_forward(diff, B, seed):
    bb = diff.backbone
    bb.eval()
    with torch.no_grad():
        _forward(diff, B, seed)
    bb.train()


def _assert_regime(bb, form, nn, where):
    """nn: qkv / out / fc1 of block 0 (of every block but the last) have no transposed shadow and recorded "nn", every other Linear - block 0's fc2, all of block 1, the head, the adaLN and
    sigma-map Linears - has one and recorded "nt".  Not nn: every Linear has one and recorded "nt"."""
    names = set(bb._lins)
    want = {f"{i}.{k}" for i in range(len(bb.blocks)) for k in ("qkv", "out", "fc1", "fc2")} | {"head"}
    if bb.time_conditioning:
        want |= {f"{i}.ada" for i in range(len(bb.blocks))} | {"head.ada", "sig0", "sig2"}
    assert names == want, names ^ want
    in_nn = {f"{i}.{k}" for i in range(len(bb.blocks) - 1) for k in NN}      # every block but the last
    for name, lin in bb._lins.items():
        w_nn = nn and name in in_nn
        assert lin.need_t == (not w_nn), f"{where}: {name}.need_t = {lin.need_t}"
        assert (lin.w16t is None) == w_nn, f"{where}: {name}.w16t is {'missing' if lin.w16t is None else 'present'}"
        assert form[name] == ("nn" if w_nn else "nt"), f"{where}: {name} recorded {form[name]!r}"


def _step(diff, opt, B, seed, log, forms, casts=None, nn=None, clip=None):
    """forward (with `casts`: exactly that many / "some" cast launches in it; with `nn`: the dgrad regime it must record), backward, optimizer step: the shadows
    must then hold the UPDATED masters.  Returns the loss."""
    bb = diff.backbone
    mark, nf = log.mark(), len(forms)
    out = _forward(diff, B, seed)
    fwd = log.forwards_since(mark)
    assert len(fwd) == 1 and fwd[0][0] == B * _PLUMB["txt_length"] and len(forms) == nf + 1, (fwd, len(forms) - nf)
    if casts is not None:
        assert (fwd[0][2] >= 1) if casts == "some" else (fwd[0][2] == casts), (casts, fwd)
    if nn is not None:
        _assert_regime(bb, forms[-1], nn, f"forward at B = {B} (seed {seed})")
    before = [l.weight.detach().clone() for l in bb._lins.values()]
    out.loss.backward()
    if clip is not None:
        torch.nn.utils.clip_grad_norm_(bb.parameters(), clip)
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert all(not torch.equal(b, l.weight.detach()) for b, l in zip(before, bb._lins.values())), "the optimizer step left a GEMM weight where it was"
    return float(out.loss.detach())


def _fused_step(diff, opt, B, seed, log, forms, casts=None, nn=None):
    loss = _step(diff, opt, B, seed, log, forms, casts, nn)
    assert_shadows_coherent(diff.backbone, f"after the fused optimizer step (seed {seed})")
    return loss


def _nn_regime_three_steps(diff, opt, log, forms):
    bb = diff.backbone
    assert opt.maintain_shadows and bb.dgrad_from_w and bb.compact_last_block and bb.recast_every_forward is True and not bb.overlap_weight_cast
    _fused_step(diff, opt, 2, 11, log, forms, casts=1, nn=True)
    assert bb.recast_every_forward is False
    _fused_step(diff, opt, 2, 12, log, forms, casts=0, nn=True)     # maintained: no recast, the forward reads what the optimizer kernel wrote
    _fused_step(diff, opt, 2, 13, log, forms, casts=0, nn=True)
    assert log.casts_since(0) == 1


# ------------------------------------------------------------------------------------------------ a. nn regime, maintained shadows
@TC
def test_nn_regime_with_maintained_shadows(tc, forms):
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    with observe_shadows() as log:
        _nn_regime_three_steps(diff, FusedAdamW(bb, **HP), log, forms)


# ------------------------------------------------------------------------------------------------ b. flip to sticky
@TC
def test_eval_forward_of_another_row_count_makes_the_transposed_shadow_sticky(tc, forms):
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _nn_regime_three_steps(diff, opt, log, forms)
        mark = log.mark()
        _eval_forward(diff, 1, 14)                                   # 128 rows: no whole tile
        assert log.forwards_since(mark) == [(128, False, 1)], log[mark:]
        _assert_regime(bb, forms[-1], False, "eval forward at B = 1")
        assert all(l.sticky_t for l in bb._lins.values())
        assert_shadows_coherent(bb, "after the eval forward at B = 1")
        # back to 256 rows: the transposed shadows stay, every dgrad reads them, and the optimizer's job table has picked up the new w16t pointers
        _fused_step(diff, opt, 2, 15, log, forms, casts=0, nn=False)
        _fused_step(diff, opt, 2, 16, log, forms, casts=0, nn=False)
        mark = log.mark()
        _eval_forward(diff, 1, 17)
        assert log.forwards_since(mark) == [(128, False, 0)], log[mark:]


@TC
def test_flip_between_the_forward_and_the_optimizer_step(tc, forms):
    """The transposed shadows appear (an eval forward at 128 rows) while a 256-row training forward that recorded "nn" is still pending: its backward runs, and the
    fused optimizer step that follows must write the NEW w16t buffers too - its job table was built when they did not exist."""
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _fused_step(diff, opt, 2, 81, log, forms, casts=1, nn=True)
        out = _forward(diff, 2, 82)
        _assert_regime(bb, forms[-1], True, "the pending training forward")
        mark = log.mark()
        _eval_forward(diff, 1, 83)
        assert log.forwards_since(mark) == [(128, False, 1)], log[mark:]
        _assert_regime(bb, forms[-1], False, "eval forward at B = 1")
        before = [l.weight.detach().clone() for l in bb._lins.values()]
        out.loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert all(not torch.equal(b, l.weight.detach()) for b, l in zip(before, bb._lins.values()))
        assert all(l.w16t is not None for l in bb._lins.values())
        assert_shadows_coherent(bb, "after the fused step that followed the flip")
        _fused_step(diff, opt, 2, 84, log, forms, casts=0, nn=False)


# ------------------------------------------------------------------------------------------------ c. two pending backwards across a flip
@functools.lru_cache(maxsize=None)
def _two_batch_reference(tc):
    """fp32 CPU oracle and its bf16 emulation (flash rounding points included) on batch A (B = 2, seed 123) and batch B (B = 1, seed 124): gradients summed.
    Computed once per model, read by both orders."""
    diff, bb = _product(tc)
    P0 = {k: v.detach().cpu().clone() for k, v in bb.named_parameters()}
    ocfg = O.OracleConfig.from_case(_case(tc))
    bufs = O.make_buffers(ocfg, lumina_rope_2d)
    res = {}
    for mode, kw in (("fp32", {}), ("bf16", dict(bf16=True, flash_rounding=True))):
        P = {k: v.clone().requires_grad_() for k, v in P0.items()}
        aux = []
        for B, seed in ((2, 123), (1, 124)):
            ob = O.update_batch(ocfg, {k: v.clone() for k, v in _batch(B, seed).items()})
            o = O.compute_loss(ocfg, P, bufs, ob, torch.Generator().manual_seed(seed), **kw)
            o.loss.backward()
            aux.append((o.aux["xt"], o.aux["move_indices"], float(o.loss.detach())))
        res[mode] = ({k: (v.grad.clone() if v.grad is not None else None) for k, v in P.items()}, aux)
    return P0, res


@TC
@pytest.mark.parametrize("order", ["BA", "AB"])
def test_two_pending_backwards_across_a_flip(tc, order, forms):
    """Forward A (256 rows) records "nn" for block 0; forward B (128 rows) then makes the transposed shadows appear (a forced recast of unchanged masters); both
    backwards run afterwards, in either order.  p.grad must be grad(A) + grad(B) of the fp32 oracle within the oracle's own bf16 floor: every parameter <= 2 x its
    floor, the worst parameter <= 1.5 x the worst floor (the scheme of test_training_step_matches_oracle_at_full_width)."""
    P0, ref = _two_batch_reference(tc)
    (g32, aux32), (g16, _) = ref["fp32"], ref["bf16"]
    diff, bb = _product(tc)
    with torch.no_grad():
        for k, p in bb.named_parameters():
            p.copy_(P0[k].to(DEV))
    name = f"shadow_lifecycle_two_backwards_{'adaln' if tc else 'no_adaln'}_{order}"
    with observe_shadows() as log:
        outA = _forward(diff, 2, 123)
        _assert_regime(bb, forms[-1], True, "forward A")
        assert torch.equal(diff._last["xt"].cpu(), aux32[0][0]) and torch.equal(diff._last["move_indices"].cpu(), aux32[0][1])
        mark = log.mark()
        outB = _forward(diff, 1, 124)
        assert log.forwards_since(mark) == [(128, False, 1)], log[mark:]
        _assert_regime(bb, forms[-1], False, "forward B")
        assert torch.equal(diff._last["xt"].cpu(), aux32[1][0]) and torch.equal(diff._last["move_indices"].cpu(), aux32[1][1])
        assert all(0 < int(a[1].sum()) < a[1].numel() for a in aux32)
        assert forms[-2]["0.qkv"] == "nn" and forms[-1]["0.qkv"] == "nt"      # the two pending backwards saw different shadow sets
        for out in ((outB, outA) if order == "BA" else (outA, outB)):
            out.loss.backward()
        torch.cuda.synchronize()
        assert_shadows_coherent(bb, "after both backwards")
    for (out, a, tag) in ((outA, aux32[0], "A"), (outB, aux32[1], "B")):
        ledger.record(name, f"loss_{tag}_rel_vs_fp32_oracle", abs(float(out.loss.detach()) - a[2]) / abs(a[2]))
    errs = []
    for k, p in bb.named_parameters():
        if g32[k] is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        errs.append((_rel(p.grad.cpu(), g32[k]), k))
    errs.sort(reverse=True)
    floor = {k: _rel(g16[k], g32[k]) for k in g32 if g32[k] is not None}
    ff = sorted(((v, k) for k, v in floor.items()), reverse=True)
    ratios = sorted(((e / max(floor[k], 1e-12), k) for e, k in errs), reverse=True)
    for e, k in errs:
        print(f"{name} {k}: grad rel-RMS {e:.3e} floor {floor[k]:.3e} ratio {e / max(floor[k], 1e-12):.2f}")
    ledger.record(name, "ref_bf16_flash_rounding_vs_fp32_grad_relrms_worst_param", ff[0][0], note=ff[0][1])
    ledger.record(name, "ref_bf16_flash_rounding_vs_fp32_grad_relrms_same_param_as_ours", floor[errs[0][1]], note=errs[0][1])
    ledger.record(name, "grad_relrms_worst_param", errs[0][0], note=errs[0][1])
    ledger.record(name, "grad_err_over_flash_rounding_floor_median_ratio", ratios[len(ratios) // 2][0])
    ledger.check(name, "grad_relrms_worst_param_over_flash_rounding_floor_worst", errs[0][0] / ff[0][0], 1.5, note=f"{errs[0][1]} vs {ff[0][1]}")
    ledger.check(name, "grad_err_over_flash_rounding_floor_worst_ratio", ratios[0][0], 2.0, note=ratios[0][1])


# ------------------------------------------------------------------------------------------------ d. EMA swap
@TC
def test_ema_swap_and_restore(tc, forms):
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _fused_step(diff, opt, 2, 21, log, forms, casts=1, nn=True)
        _fused_step(diff, opt, 2, 22, log, forms, casts=0, nn=True)
        trained = {k: v.detach().clone() for k, v in bb.named_parameters()}
        mark = log.mark()
        opt.ema_store_and_copy()
        assert log[mark:] == [(None, True, 1)], log[mark:]
        assert all(torch.equal(p.detach(), opt.ema[id(p)]) for p in opt.params)
        assert all(not torch.equal(trained[k], v.detach()) for k, v in bb.named_parameters() if k.endswith("attn_qkv.weight"))
        assert_shadows_coherent(bb, "with the EMA weights")
        mark = log.mark()
        _eval_forward(diff, 2, 23)
        assert log.forwards_since(mark) == [(256, False, 0)], log[mark:]
        mark = log.mark()
        opt.ema_restore()
        assert log[mark:] == [(None, True, 1)], log[mark:]
        assert all(torch.equal(trained[k], v.detach()) for k, v in bb.named_parameters())
        assert_shadows_coherent(bb, "after ema_restore")
        _fused_step(diff, opt, 2, 24, log, forms, casts=0, nn=True)


# ------------------------------------------------------------------------------------------------ e. checkpoint and optimizer reload
@TC
def test_checkpoint_and_optimizer_reload(tc, forms, tmp_path):
    from unidisc_amd import FusedAdamW
    from unidisc_amd.checkpoint import load_backbone_checkpoint, save_backbone_checkpoint

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _fused_step(diff, opt, 2, 31, log, forms, casts=1, nn=True)
        save_backbone_checkpoint(bb, str(tmp_path))
        saved = {k: v.detach().clone() for k, v in bb.named_parameters()}
        sd = {k: ([t.clone() for t in v] if isinstance(v, list) else v) for k, v in opt.state_dict().items()}
        _fused_step(diff, opt, 2, 32, log, forms, casts=0, nn=True)
        _fused_step(diff, opt, 2, 33, log, forms, casts=0, nn=True)
        before = {k: v.detach().clone() for k, v in bb.named_parameters()}
        load_backbone_checkpoint(bb, str(tmp_path))
        opt.load_state_dict(sd)
        names = {id(p): k for k, p in bb.named_parameters()}
        for k, v in bb.named_parameters():
            assert torch.equal(v.detach(), saved[k]), k
        for lin in bb._lins.values():
            assert not torch.equal(before[names[id(lin.weight)]], lin.weight.detach()), names[id(lin.weight)]
        assert opt.step_count == 1
        _fused_step(diff, opt, 2, 34, log, forms, casts="some", nn=True)   # the observer holds this forward's shadows to the LOADED masters
        _fused_step(diff, opt, 2, 35, log, forms, casts=0, nn=True)


# ------------------------------------------------------------------------------------------------ f. foreign writers
@TC
def test_foreign_writers(tc, forms):
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _fused_step(diff, opt, 2, 41, log, forms, casts=1, nn=True)
        _fused_step(diff, opt, 2, 42, log, forms, casts=0, nn=True)
        assert bb.recast_every_forward is False
        _step(diff, torch.optim.SGD(bb.parameters(), lr=1e-2), 2, 43, log, forms, casts=0, nn=True)     # in-place writes: the versions move
        _fused_step(diff, opt, 2, 44, log, forms, casts="some", nn=True)                              # ... and this forward recasts
        _fused_step(diff, opt, 2, 45, log, forms, casts=0, nn=True)
        # the documented contract: a p.data write, which no version counter sees, followed by invalidate_shadows()
        lin = bb._lins["0.fc1"]
        v = lin.weight._version
        lin.weight.data.mul_(1.01)
        assert lin.weight._version == v
        bb.invalidate_shadows()
        mark = log.mark()
        _eval_forward(diff, 2, 46)
        assert log.forwards_since(mark) == [(256, False, 1)], log[mark:]
        _fused_step(diff, opt, 2, 47, log, forms, casts=0, nn=True)


# ------------------------------------------------------------------------------------------------ g. sampling between steps
@TC
def test_sampling_between_fused_steps(tc, forms):
    from unidisc_amd import FusedAdamW

    diff, bb = _product(tc)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _fused_step(diff, opt, 2, 51, log, forms, casts=1, nn=True)
        bb.eval()
        mark = log.mark()
        x, nfe = diff.sample(num_steps=3, batch_size=2, seed=5, predictor="maskgit", return_nfe=True)
        bb.train()
        assert tuple(x.shape) == (2, _PLUMB["txt_length"]) and not bool((x == diff.mask_index).any())
        seen = log.forwards_since(mark)
        assert len(seen) == nfe == 4 and all(e == (256, False, 0) for e in seen), (nfe, seen)     # every sampler forward under the observer, none of them recasts
        _fused_step(diff, opt, 2, 52, log, forms, casts=0, nn=True)
        _fused_step(diff, opt, 2, 53, log, forms, casts=0, nn=True)


def test_kv_cached_sampling_between_fused_steps():
    """The cached paths (`reset_kv_cache`, the decode step: `_refresh_shadows_now`) need a causal backbone: the AR baseline on the `ar_c_large` golden case.  A
    KV-cached sampling run between fused optimizer steps: its shadow refreshes are observed like every other, launch no cast, and the training steps around it stay
    coherent."""
    from ar_utils import ArGolden, build_ar_product
    from unidisc_amd import FusedAdamW

    g = ArGolden("ar_c_large")
    diff = build_ar_product(g, DEV)
    bb = diff.backbone
    opt = FusedAdamW(bb, **HP)
    L = diff.config.model.length
    mod = torch.zeros(2, L, dtype=torch.int64, device=DEV)
    mod[:, diff.static_img_sl] = 1

    def step(seed):
        torch.manual_seed(seed)
        out = diff.training_step(g.batch(), seed)
        out.loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert_shadows_coherent(bb, f"after the fused optimizer step (seed {seed})")

    with observe_shadows() as log:
        step(61)
        bb.eval()
        mark = log.mark()
        x, _ = diff._ar_sampler(2, modality=mod, seed=5, bos_token_id=3)
        assert tuple(x.shape) == (2, L) and not bool((x == diff.mask_index).any())
        # the sampler: reset_kv_cache fixes the shadows for the whole run (rows = None), the prefill is an engine forward
        assert [e for e in log[mark:] if e[0] is None] == [(None, False, 0)] and len(log.forwards_since(mark)) == 1, log[mark:]
        assert log.casts_since(mark) == 0
        # forward(start_pos = ...): a prefill of four tokens, then two decode steps, each of which fixes its shadows itself
        mark = log.mark()
        with torch.no_grad():
            bb.reset_kv_cache(batch_size=2, seq_len=L, dtype=torch.bfloat16, device=DEV, modality=mod)
            bb(x[:, :4], None, modality=mod[:, :4], start_pos=0)
            for p in (4, 5):
                bb(x[:, p:p + 1], None, modality=mod[:, p:p + 1], start_pos=p)
            bb.reset_kv_cache(set_to_none=True)
        bb.train()
        assert [e for e in log[mark:] if e[0] is None] == [(None, False, 0)] * 3 and len(log.forwards_since(mark)) == 1, log[mark:]
        assert log.casts_since(mark) == 0
        mark = log.mark()
        step(62)
        assert log.casts_since(mark) == 0


# ------------------------------------------------------------------------------------------------ h. side-stream cast
@pytest.mark.parametrize("tc,n_blocks", [(True, 2), (False, 2), (True, 4)], ids=["adaln", "no_adaln", "adaln_4blocks"])
def test_side_stream_cast_is_awaited_and_changes_nothing(tc, n_blocks, forms):
    """`overlap_weight_cast`: the per-forward recast (torch.optim.AdamW maintains no shadows) runs on a side stream in one launch per part - one part at two blocks,
    two at four.  Every queued group is awaited before use (`_cast_events` is empty after each forward), the shadows are the bf16 of the masters, and the losses are
    those of the same run with the flag off."""
    losses = {}
    for overlap in (True, False):
        diff, bb = _product(tc, n_blocks)
        bb.overlap_weight_cast = overlap
        opt = torch.optim.AdamW(bb.parameters(), lr=2e-3, eps=1e-3, weight_decay=0.01)
        parts = (2 if n_blocks == 4 else 1) if overlap else 1
        losses[overlap] = []
        with observe_shadows() as log:
            for i, seed in enumerate((71, 72, 73)):
                mark = log.mark()
                out = _forward(diff, 2, seed)
                assert bb._cast_events == {}, sorted(bb._cast_events)
                fwd = log.forwards_since(mark)
                # the first forward builds the shadows (a forced cast on the compute stream); each later one recasts without force: on the side stream with the flag
                assert fwd == [(256, False, 1 if i == 0 else parts)], (i, fwd)
                assert getattr(bb, "_cast_stream", None) is not None if (overlap and i > 0) else True
                _assert_regime(bb, forms[-1], True, f"forward {i}")
                assert_shadows_coherent(bb, f"after forward {i}")
                out.loss.backward()
                torch.nn.utils.clip_grad_norm_(bb.parameters(), 0.5)
                opt.step()
                opt.zero_grad(set_to_none=True)
                assert bb.recast_every_forward is True
                losses[overlap].append(float(out.loss.detach()))
        if not overlap:
            assert getattr(bb, "_cast_stream", None) is None
    assert all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(losses[True], losses[False])), losses
