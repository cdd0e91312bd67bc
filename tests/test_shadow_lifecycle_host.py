"""The weight-shadow cache across the training lifecycle, on the CPU with kernel doubles (tests/fake_kernels.py): the version check, `invalidate_shadows`,
`recast_every_forward` and the optimizer's maintained shadows, under the observer of tests/shadow_utils.py - after every `refresh_weight_shadows` call each
shadow must be, exactly, torch's bf16 cast of its master.  The `need_t` / `sticky_t` logic is gated on `.is_cuda` and is covered by
tests/test_gpu_shadow_lifecycle.py.  The last tests show that the checker fails when the cache is made stale on purpose."""
import pytest
import torch

import fake_kernels
from golden_utils import Golden
from product_utils import build_product
from shadow_utils import assert_shadows_coherent, observe_shadows

CASES = ["c_large", "d_adaln_mm"]
HP = dict(lr=2e-3, weight_decay=0.01, max_grad_norm=0.5, ema_decay=0.999)


@pytest.fixture()
def fake_k(monkeypatch):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod, optim as optim_mod, zero as zero_mod

    for mod in (dit_mod, diff_mod, optim_mod, zero_mod):
        monkeypatch.setattr(mod, "K", fake_kernels)
    return fake_kernels


def _product(name):
    g = Golden(name)
    diff = build_product(g, device="cpu")
    diff.rng_device = "cpu"
    return g, diff, diff.backbone


def _forward(diff, g, seed):
    torch.manual_seed(seed)
    return diff.training_step(g.batch(), seed)


def _step(diff, g, opt, seed, log=None, casts=None):
    """forward (with `casts`: exactly that many / "some" cast launches in it), backward, optimizer step; the shadows must then hold the UPDATED masters"""
    mark = log.mark() if log is not None else 0
    out = _forward(diff, g, seed)
    if casts is not None:
        fwd = log.forwards_since(mark)
        assert len(fwd) == 1, fwd
        assert (fwd[0][2] >= 1) if casts == "some" else (fwd[0][2] == casts), (casts, fwd)
    before = [l.weight.detach().clone() for l in diff.backbone._lins.values()]
    out.loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    assert any(not torch.equal(b, l.weight.detach()) for b, l in zip(before, diff.backbone._lins.values())), "the optimizer step moved no GEMM weight"
    assert_shadows_coherent(diff.backbone, f"after optimizer step (seed {seed})")


def _eval_forward(diff, g, seed):
    bb = diff.backbone
    bb.eval()
    with torch.no_grad():
        _forward(diff, g, seed)
    bb.train()


def _masters(bb):
    return {k: v.detach().clone() for k, v in bb.named_parameters()}


# ------------------------------------------------------------------------------------------------ the scenarios
@pytest.mark.parametrize("name", CASES)
def test_fused_steps_maintain_the_shadows_without_recasting(name, fake_k):
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product(name)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        assert bb.recast_every_forward is True
        _step(diff, g, opt, 11, log, casts=1)           # no optimizer has run yet: the forward casts
        assert bb.recast_every_forward is False
        _step(diff, g, opt, 12, log, casts=0)           # maintained: the shadows the forward reads are the ones the optimizer kernel wrote
        _step(diff, g, opt, 13, log, casts=0)
    assert log.casts_since(0) == 1 and len(log) == 3


@pytest.mark.parametrize("name", CASES)
def test_ema_swap_and_restore(name, fake_k):
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product(name)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _step(diff, g, opt, 21, log)
        _step(diff, g, opt, 22, log, casts=0)
        trained = _masters(bb)
        mark = log.mark()
        opt.ema_store_and_copy()
        assert all(torch.equal(p.detach(), opt.ema[id(p)]) for p in opt.params)
        assert any(not torch.equal(trained[k], v.detach()) for k, v in bb.named_parameters())
        assert log.casts_since(mark) >= 1
        assert_shadows_coherent(bb, "with the EMA weights")
        _eval_forward(diff, g, 23)
        mark = log.mark()
        opt.ema_restore()
        assert all(torch.equal(trained[k], v.detach()) for k, v in bb.named_parameters())
        assert log.casts_since(mark) >= 1
        assert_shadows_coherent(bb, "after ema_restore")
        _step(diff, g, opt, 24, log)
        _step(diff, g, opt, 25, log, casts=0)


@pytest.mark.parametrize("name", CASES)
def test_checkpoint_and_optimizer_reload(name, fake_k, tmp_path):
    from unidisc_amd import FusedAdamW
    from unidisc_amd.checkpoint import load_backbone_checkpoint, save_backbone_checkpoint

    g, diff, bb = _product(name)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _step(diff, g, opt, 31, log)
        save_backbone_checkpoint(bb, str(tmp_path))
        saved, sd = _masters(bb), {k: ([t.clone() for t in v] if isinstance(v, list) else v) for k, v in opt.state_dict().items()}
        _step(diff, g, opt, 32, log, casts=0)
        _step(diff, g, opt, 33, log, casts=0)
        before = _masters(bb)
        load_backbone_checkpoint(bb, str(tmp_path))
        opt.load_state_dict(sd)
        for k, v in bb.named_parameters():
            assert torch.equal(v.detach(), saved[k]), k
        names = {id(p): k for k, p in bb.named_parameters()}
        for lin in bb._lins.values():   # every GEMM weight went back: the shadows of the steps since are stale until the next forward
            assert not torch.equal(before[names[id(lin.weight)]], lin.weight.detach()), names[id(lin.weight)]
        assert opt.step_count == 1
        _step(diff, g, opt, 34, log, casts="some")      # the forward after the load rebuilds the shadows from the loaded masters (the observer checks them)
        _step(diff, g, opt, 35, log, casts=0)


def _foreign_sgd_step(diff, g, seed):
    """one torch.optim.SGD step on the backbone's parameters: in-place writes that bump the tensor versions and know nothing of the shadows"""
    bb = diff.backbone
    out = _forward(diff, g, seed)
    out.loss.backward()
    before = [l.weight.detach().clone() for l in bb._lins.values()]
    torch.optim.SGD(bb.parameters(), lr=1e-1).step()
    bb.zero_grad(set_to_none=True)
    assert all(not torch.equal(b, l.weight.detach()) for b, l in zip(before, bb._lins.values()))


def _data_write(bb):
    """the documented contract: a `p.data` write (the version counter does not see it) followed by invalidate_shadows()"""
    lin = bb._lins["0.fc1"]
    v = lin.weight._version
    lin.weight.data.mul_(1.01)
    assert lin.weight._version == v
    return lin


@pytest.mark.parametrize("name", CASES)
def test_foreign_writers(name, fake_k):
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product(name)
    opt = FusedAdamW(bb, **HP)
    with observe_shadows() as log:
        _step(diff, g, opt, 41, log)
        _step(diff, g, opt, 42, log, casts=0)
        assert bb.recast_every_forward is False
        _foreign_sgd_step(diff, g, 43)
        _step(diff, g, opt, 44, log, casts="some")      # the versions moved: this forward recasts (the observer checks the result)
        _step(diff, g, opt, 45, log, casts=0)
        _data_write(bb)
        bb.invalidate_shadows()
        mark = log.mark()
        _eval_forward(diff, g, 46)
        assert log.casts_since(mark) >= 1
        _step(diff, g, opt, 47, log, casts=0)


@pytest.mark.parametrize("name", CASES)
def test_sharded_adamw_on_one_rank_maintains_the_shadows(name, fake_k, tmp_path):
    import torch.distributed as dist

    from unidisc_amd import zero as zero_mod

    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        g, diff, bb = _product(name)
        sync = zero_mod.wrap_sharded(bb, force_single_rank=False)
        assert not sync.active
        opt = zero_mod.ShardedAdamW(bb, sync, **HP)
        with observe_shadows() as log:
            _step(diff, g, opt, 51, log, casts=1)
            _step(diff, g, opt, 52, log, casts=0)
            opt.ema_store_and_copy()
            assert_shadows_coherent(bb, "with the EMA weights")
            _eval_forward(diff, g, 53)
            opt.ema_restore()
            assert_shadows_coherent(bb, "after ema_restore")
            _step(diff, g, opt, 54, log, casts=0)
            opt.load_state_dict(opt.state_dict())
            _step(diff, g, opt, 55, log, casts="some")
            _step(diff, g, opt, 56, log, casts=0)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ the checker must be able to fail
def _lifecycle(diff, g, opt, tmp_path, monkeypatch, mutate=None):
    """The scenarios above in one run: fused steps, a checkpoint reload, a foreign optimizer, a `p.data` write.  `mutate` breaks one link of it."""
    from unidisc_amd import dit as dit_mod
    from unidisc_amd.checkpoint import load_backbone_checkpoint, save_backbone_checkpoint

    bb = diff.backbone
    with observe_shadows() as log:
        if mutate == "optimizer_leaves_w16":
            # the optimizer kernel updates the master, the moments, the EMA and the transposed shadow - not w16 (positional argument 12)
            orig = fake_kernels.adamw_step_shadow
            monkeypatch.setattr(fake_kernels, "adamw_step_shadow", lambda *a, **kw: orig(*a[:12], None, *a[13:], **kw))
        _step(diff, g, opt, 61, log)
        _step(diff, g, opt, 62, log, casts=0)
        save_backbone_checkpoint(bb, str(tmp_path))
        _step(diff, g, opt, 63, log, casts=0)
        # checkpoint load, then an eval forward: nothing but the shadow cache's own bookkeeping stands between the loaded masters and the GEMMs
        with monkeypatch.context() as mp:
            if mutate in ("load_without_invalidate", "load_without_invalidate_or_versions"):
                mp.setattr(dit_mod.DIT, "invalidate_shadows", lambda self: None)
            load_backbone_checkpoint(bb, str(tmp_path))
        if mutate == "load_without_invalidate_or_versions":
            monkeypatch.setattr(bb, "_shadow_versions", [l.weight._version for l in bb._lins.values()])
        mark = log.mark()
        _eval_forward(diff, g, 64)
        assert log.casts_since(mark) >= 1
        _step(diff, g, opt, 65, log, casts=0)
        # a torch optimizer in between, then an eval forward
        _foreign_sgd_step(diff, g, 66)
        if mutate == "versions_forced_equal":
            monkeypatch.setattr(bb, "_shadow_versions", [l.weight._version for l in bb._lins.values()])
        mark = log.mark()
        _eval_forward(diff, g, 67)
        assert log.casts_since(mark) >= 1
        # a p.data write
        _data_write(bb)
        if mutate != "data_write_without_invalidate":
            bb.invalidate_shadows()
        _eval_forward(diff, g, 68)
        _step(diff, g, opt, 69, log, casts=0)
    return log


def test_unmutated_lifecycle_passes(fake_k, tmp_path, monkeypatch):
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product("c_large")
    _lifecycle(diff, g, FusedAdamW(bb, **HP), tmp_path, monkeypatch)


@pytest.mark.parametrize("mutate,message", [
    ("optimizer_leaves_w16", r"w16 is not the bf16 of its master"),                       # the optimizer kernel updates p but not w16
    ("versions_forced_equal", r"w16 is not the bf16 of its master"),                      # the version comparison sees nothing after a torch.optim step
    ("load_without_invalidate_or_versions", r"w16 is not the bf16 of its master"),        # a checkpoint load neither invalidate_shadows nor the versions report
    ("data_write_without_invalidate", r"0\.fc1\.w16 is not the bf16 of its master"),      # the documented contract, broken by the caller
])
def test_checker_fails_on_a_stale_cache(mutate, message, fake_k, tmp_path, monkeypatch):
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product("c_large")
    with pytest.raises(AssertionError, match=message):
        _lifecycle(diff, g, FusedAdamW(bb, **HP), tmp_path, monkeypatch, mutate=mutate)


def test_checkpoint_load_is_also_caught_by_the_version_counters(fake_k, tmp_path, monkeypatch):
    """`DIT.invalidate_shadows` as a no-op during `load_backbone_checkpoint` does NOT leave the cache stale: `nn.Module.load_state_dict` copies into the parameters in
    place, which bumps their version counters, and the next forward recasts on that (asserted inside `_lifecycle`: at least one cast launch in that forward, and the
    observer finds the shadows equal to the loaded masters).  The call in the loader is a second guard for loaders that write around the counters; the case where
    neither guard reports the load is `load_without_invalidate_or_versions` above, and there the checker fails."""
    from unidisc_amd import FusedAdamW

    g, diff, bb = _product("c_large")
    _lifecycle(diff, g, FusedAdamW(bb, **HP), tmp_path, monkeypatch, mutate="load_without_invalidate")
