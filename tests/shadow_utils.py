"""The bf16 weight shadows (`_Lin.w16`, `_Lin.w16t`) as a cache of the fp32 masters: the invariant every forward relies on, and an observer that checks it
at the moment a forward fixes its shadows.  Shared by tests/test_shadow_lifecycle_host.py (CPU, kernel doubles) and tests/test_gpu_shadow_lifecycle.py.

The reference of every comparison is torch's own round-to-nearest-even cast of the master weight; nothing of the code under test is in it, and every
comparison is exact (`torch.equal`)."""
import contextlib

import torch

BF16 = torch.bfloat16


def assert_shadows_coherent(backbone, where):
    """Every `_Lin` of `backbone._lins`: w16[:out] is bf16(master) and its padding rows are zero; a transposed shadow, where there is one, is bf16(masterᵀ) with
    zero padding columns; there is a transposed shadow exactly where `need_t` says so; a sticky layer needs one."""
    lins = backbone._lins
    assert lins, f"{where}: the backbone has no weight shadows yet"
    if next(iter(lins.values())).weight.is_cuda:
        torch.cuda.synchronize()
    for name, lin in lins.items():
        w = lin.weight.detach()
        assert lin.w16 is not None, f"{where}: {name}.w16 is missing"
        assert tuple(lin.w16.shape) == (lin.outp, lin.inp), f"{where}: {name}.w16 has shape {tuple(lin.w16.shape)}"
        assert torch.equal(lin.w16[: lin.out], w.to(BF16)), f"{where}: {name}.w16 is not the bf16 of its master"
        assert not bool(lin.w16[lin.out:lin.outp].any()), f"{where}: {name}.w16 has non-zero padding rows"
        if lin.w16t is not None:
            assert tuple(lin.w16t.shape) == (lin.inp, lin.outp), f"{where}: {name}.w16t has shape {tuple(lin.w16t.shape)}"
            assert torch.equal(lin.w16t[:, : lin.out], w.t().to(BF16)), f"{where}: {name}.w16t is not the bf16 of its transposed master"
            assert not bool(lin.w16t[:, lin.out:].any()), f"{where}: {name}.w16t has non-zero padding columns"
        assert (lin.w16t is None) == (not lin.need_t), f"{where}: {name} need_t = {lin.need_t} but w16t is {'missing' if lin.w16t is None else 'present'}"
        assert lin.need_t or not lin.sticky_t, f"{where}: {name} is sticky_t without need_t"


class ShadowLog(list):
    """One `(rows, force, casts)` per `refresh_weight_shadows` call: the row count the forward passed (None: the cached paths, the optimizer's forced
    refreshes), its `force` argument, the number of `K.cast_transpose_multi` launches inside the call."""

    def mark(self):
        return len(self)

    def casts_since(self, mark):
        return sum(c for _, _, c in self[mark:])

    def forwards_since(self, mark):
        """the calls a forward made (engine forwards pass their row count)"""
        return [e for e in self[mark:] if e[0] is not None]


@contextlib.contextmanager
def observe_shadows(check=True):
    """Wraps the METHOD `DIT.refresh_weight_shadows`, so every forward - the engine forward, the cached and decode paths through `_refresh_shadows_now`,
    `reset_kv_cache` - and every forced refresh of an optimizer is seen at the moment its shadows are fixed.  After each call the invariant runs
    (`check=False`: log only) and the call is logged.  Yields the `ShadowLog`."""
    import unidisc_amd.dit as dit_mod

    log = ShadowLog()
    orig = dit_mod.DIT.refresh_weight_shadows

    def observed(self, force=False, rows=None):
        K = dit_mod.K
        launch, n = K.cast_transpose_multi, [0]

        def counted(jobs):
            n[0] += 1
            return launch(jobs)

        K.cast_transpose_multi = counted
        try:
            out = orig(self, force=force, rows=rows)
        finally:
            K.cast_transpose_multi = launch
        log.append((rows, bool(force), n[0]))
        if check:
            assert_shadows_coherent(self, f"refresh_weight_shadows(force={force}, rows={rows}), call {len(log)}")
        return out

    dit_mod.DIT.refresh_weight_shadows = observed
    try:
        yield log
    finally:
        dit_mod.DIT.refresh_weight_shadows = orig
