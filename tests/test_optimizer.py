"""FusedAdamW (+ global-norm clipping, bf16 shadow maintenance) against torch.optim.AdamW + clip_grad_norm_, which is what
the reference's loop runs (model_setup.py:385-424, model.py:1516-1545).  CPU part: the host logic with kernel doubles; GPU part: the HIP
kernels themselves."""
import copy
import math
import struct

import pytest
import torch

import fake_kernels
import ledger
import optim_cases as OC
import optim_ref
from golden_utils import Golden, rel_err
from product_utils import build_product

DEV = "cuda"


def _torch_reference_steps(params, grads_per_step, lr, betas, eps, wd, max_norm):
    ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        opt.step()
    return [p.detach() for p in ps], norms


@pytest.fixture()
def fake_k(monkeypatch):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod, optim as optim_mod

    monkeypatch.setattr(dit_mod, "K", fake_kernels)
    monkeypatch.setattr(diff_mod, "K", fake_kernels)
    monkeypatch.setattr(optim_mod, "K", fake_kernels)
    return fake_kernels


@pytest.mark.parametrize("max_norm", [None, 0.05])
def test_fused_adamw_host_logic_matches_torch(fake_k, max_norm):
    from unidisc_amd import FusedAdamW

    g = Golden("c_large")
    diff = build_product(g, device="cpu")
    diff.rng_device = "cpu"
    bb = diff.backbone
    ref_model = copy.deepcopy(bb)
    opt = FusedAdamW(bb, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01, max_grad_norm=max_norm)
    ref_opt = torch.optim.AdamW(ref_model.parameters(), lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    for step in range(3):
        torch.manual_seed(100 + step)
        out = diff.training_step(g.batch(), step)
        out.loss.backward()
        for (n, p), (_, q) in zip(bb.named_parameters(), ref_model.named_parameters()):
            q.grad = p.grad.detach().clone() if p.grad is not None else None
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_(ref_model.parameters(), max_norm)
        ref_opt.step()
        opt.step()
        if max_norm is not None:
            assert torch.allclose(opt.grad_norm.reshape(()), tn, rtol=1e-5)
        opt.zero_grad()
        ref_opt.zero_grad()
        for (n, p), (_, q) in zip(bb.named_parameters(), ref_model.named_parameters()):
            assert torch.allclose(p, q, rtol=2e-5, atol=1e-7), (step, n)
        # the optimizer keeps the bf16 shadows current and switches the per-forward re-cast off
        assert bb.recast_every_forward is False
        for lin in bb._lins.values():
            assert torch.equal(lin.w16[: lin.out], lin.weight.detach().bfloat16())
            assert torch.equal(lin.w16t[:, : lin.out], lin.weight.detach().t().bfloat16())
    assert opt.step_count == 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 4096, 100003])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_kernel_matches_torch(n, clip):
    from unidisc_amd import kernels as K

    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (10.0 if clip else 1.0) for _ in range(4)]
    lr, betas, eps, wd, mx = 3e-3, (0.9, 0.99), 1e-8, 0.05, (1.0 if clip else None)
    (ref,), norms = _torch_reference_steps([p0], [[g] for g in grads], lr, betas, eps, wd, mx)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gsq = torch.zeros(1, device=DEV)
    for t, g in enumerate(grads, 1):
        gd = g.to(DEV)
        if clip:
            K.sumsq(gd, gsq)
            assert torch.allclose(gsq.sqrt().cpu().reshape(()), norms[t - 1], rtol=1e-5)
        K.adamw_step(p, gd, m, v, lr, betas[0], betas[1], eps, wd, t, gsq if clip else None, mx)
    assert torch.allclose(p.cpu(), ref, rtol=2e-5, atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("R,C,pad", [(64, 64, 0), (200, 328, 0), (2048, 512, 0), (97, 130, 31), (48, 2048, 80)])
def test_adamw_shadow_kernel(R, C, pad):
    from unidisc_amd import kernels as K

    gen = torch.Generator().manual_seed(R * 1000 + C)
    p0 = torch.randn(R, C, generator=gen)
    grads = [torch.randn(R, C, generator=gen) for _ in range(3)]
    lr, betas, eps, wd = 1e-2, (0.9, 0.999), 1e-8, 0.0
    (ref,), _ = _torch_reference_steps([p0], [[g] for g in grads], lr, betas, eps, wd, None)
    Rp = R + pad
    p, m, v = p0.clone().to(DEV), torch.zeros(R, C, device=DEV), torch.zeros(R, C, device=DEV)
    w16, w16t = torch.zeros((Rp, C), dtype=torch.bfloat16, device=DEV), torch.zeros((C, Rp), dtype=torch.bfloat16, device=DEV)
    for t, g in enumerate(grads, 1):
        K.adamw_step_shadow(p, g.to(DEV), m, v, lr, betas[0], betas[1], eps, wd, t, None, None, w16, w16t)
    assert torch.allclose(p.cpu(), ref, rtol=2e-5, atol=1e-7)
    assert torch.equal(w16[:R].cpu(), p.cpu().bfloat16()) and torch.equal(w16t[:, :R].cpu(), p.cpu().t().bfloat16())
    assert not w16[R:].any() and not w16t[:, R:].any()  # padding rows / columns stay zero


@pytest.mark.gpu
def test_training_steps_with_fused_adamw_match_torch_adamw_with_recast():
    """Three optimisation steps of the product model on the GPU: FusedAdamW (shadows maintained, no re-cast) vs torch.optim.AdamW +
    clip_grad_norm_ with the forward re-casting the weights -- same losses, same parameters.  (eps = 1e-3: with the default 1e-8 Adam
    normalises gradients that are pure accumulation-order noise, e.g. the k-norm bias whose true gradient is zero, to +-lr steps, and two
    runs of the SAME code then differ in those parameters.)"""
    from unidisc_amd import FusedAdamW

    g = Golden("c_large")
    res = []
    for fused in (True, False):
        diff = build_product(g, device=DEV)
        bb = diff.backbone
        batch = {k: v.to(DEV) for k, v in g.batch().items()}
        if fused:
            opt = FusedAdamW(bb, lr=2e-3, eps=1e-3, weight_decay=0.01, max_grad_norm=0.5)
        else:
            opt = torch.optim.AdamW(bb.parameters(), lr=2e-3, eps=1e-3, weight_decay=0.01)
        losses = []
        for step in range(3):
            torch.manual_seed(7 + step)
            out = diff.training_step(batch, step)
            out.loss.backward()
            if not fused:
                torch.nn.utils.clip_grad_norm_(bb.parameters(), 0.5)
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(float(out.loss))
        res.append((losses, {n: p.detach().float().cpu().clone() for n, p in bb.named_parameters()}))
    (l1, p1), (l0, p0) = res
    assert all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(l1, l0)), (l1, l0)
    for n in p0:
        assert rel_err(p1[n], p0[n]) < 2e-3, n


# ------------------------------------------------------------------------------------------------ parameter EMA (models/ema.py:44-53)
class _RefEMA:
    """The reference's ExponentialMovingAverage.update / copy_to / store / restore arithmetic, restated for the check."""

    def __init__(self, params, decay, use_num_updates=True):
        self.decay, self.n = decay, 0 if use_num_updates else None
        self.shadow = [p.clone().detach() for p in params]

    def update(self, params):
        d = self.decay
        if self.n is not None:
            self.n += 1
            d = min(d, (1 + self.n) / (10 + self.n))
        for s, p in zip(self.shadow, params):
            s.sub_((1.0 - d) * (s - p))


def test_fused_adamw_ema_host_logic(fake_k):
    from unidisc_amd import FusedAdamW

    def net():
        torch.manual_seed(3)
        return torch.nn.Sequential(torch.nn.Linear(12, 20), torch.nn.LayerNorm(20), torch.nn.Linear(20, 7))

    def grads(mod, seed):
        g = torch.Generator().manual_seed(seed)
        for p in mod.parameters():
            p.grad = torch.randn(p.shape, generator=g)

    model, ref = net(), net()
    opt = FusedAdamW(model, lr=1e-2, weight_decay=0.01, max_grad_norm=0.05, maintain_shadows=False, ema_decay=0.999)
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    ema = _RefEMA(list(ref.parameters()), 0.999)
    for it in range(12):
        grads(model, 50 + it)
        grads(ref, 50 + it)
        opt.step()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.05)
        topt.step()
        ema.update(list(ref.parameters()))
    for p, s_ in zip(opt.params, ema.shadow):
        torch.testing.assert_close(opt.ema[id(p)], s_, rtol=2e-5, atol=1e-7)
    assert opt.ema_num_updates == 12
    # store / copy_to / restore
    before = [p.detach().clone() for p in opt.params]
    opt.ema_store_and_copy()
    for p in opt.params:
        assert torch.equal(p, opt.ema[id(p)])
    opt.ema_restore()
    for p, b in zip(opt.params, before):
        assert torch.equal(p, b)
    # state dict round trip keeps the EMA and its warm-up counter
    opt2 = FusedAdamW(model, lr=1e-2, maintain_shadows=False, ema_decay=0.999)
    opt2.load_state_dict(opt.state_dict())
    assert opt2.ema_num_updates == 12 and all(torch.equal(opt2.ema[id(p)], opt.ema[id(p)]) for p in opt.params)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 4096, 100003])
def test_adamw_kernel_ema(n):
    from unidisc_amd import kernels as K
    g = torch.Generator().manual_seed(n)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m, v, e = torch.zeros(n), torch.zeros(n), torch.randn(n, generator=g)
    pd, gd, md, vd, ed = (t.clone().cuda() for t in (p, gr, m, v, e))
    for step in (1, 2, 3):
        K.adamw_step(pd, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, ema=ed, ema_decay=0.9 + 0.03 * step)
        fake_kernels.adamw_step(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, ema=e, ema_decay=0.9 + 0.03 * step)
    torch.testing.assert_close(pd.cpu(), p, rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(ed.cpu(), e, rtol=2e-6, atol=1e-7)   # fp32 arithmetic in the same order: rounding-level agreement


@pytest.mark.gpu
@pytest.mark.parametrize("R,C", [(64, 64), (200, 328), (97, 130)])
def test_adamw_shadow_kernel_ema(R, C):
    from unidisc_amd import kernels as K
    g = torch.Generator().manual_seed(R * 1000 + C)
    p, gr, e = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    m, v = torch.zeros(R, C), torch.zeros(R, C)
    w16, w16t = torch.zeros(R, C, dtype=torch.bfloat16), torch.zeros(C, R, dtype=torch.bfloat16)
    pd, gd, md, vd, ed, w16d, w16td = (t.clone().cuda() for t in (p, gr, m, v, e, w16, w16t))
    K.adamw_step_shadow(pd, gd, md, vd, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, w16d, w16td, ema=ed, ema_decay=0.95)
    fake_kernels.adamw_step_shadow(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, w16, w16t, ema=e, ema_decay=0.95)
    torch.testing.assert_close(ed.cpu(), e, rtol=2e-6, atol=1e-7)
    assert torch.equal(w16d.cpu(), pd.cpu().bfloat16()) and torch.equal(w16td.cpu(), pd.cpu().t().bfloat16())


# ------------------------------------------------------------------------------------------------ the step as the product runs it
@pytest.mark.gpu
def test_product_step_matches_float64_on_its_own_gradients(monkeypatch):
    """Four FusedAdamW steps of the c_large product model on the GPU (clipping, weight decay, EMA with warm-up, shadows maintained, default eps = 1e-8).  After every
    backward the gradients are copied to the CPU and a float64 optimizer (tests/optim_ref.py) advances on THOSE gradients, so the model's bf16 noise is not in the
    comparison: p, both moments, the EMA and the pre-clip norm are held to the kernel-level bound of tests/optim_cases.py (factor x max(fp32 CPU restatement's error,
    half an fp32 ulp), both chains running from the same start on the same gradients).  Step 2 runs on fresh clones of the gradients (per-tensor sum of squares, job
    tables rebuilt), step 3 with one parameter without a gradient (it must not move)."""
    from unidisc_amd import FusedAdamW, optim as optim_mod

    g = Golden("c_large")
    diff = build_product(g, device=DEV)
    bb = diff.backbone
    batch = {k: v.to(DEV) for k, v in g.batch().items()}
    hp = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    max_norm, decay = 0.5, 0.999
    opt = FusedAdamW(bb, lr=hp["lr"], weight_decay=hp["weight_decay"], max_grad_norm=max_norm, ema_decay=decay)
    assert opt.maintain_shadows and opt.eps == 1e-8 and opt.betas == hp["betas"]
    calls = {}
    for name in ("sumsq", "adamw_step", "adamw_step_shadow", "adamw_step_multi", "adamw_step_shadow_multi"):
        def counted(*a, _f=getattr(optim_mod.K, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(optim_mod.K, name, counted)

    names = {id(p): n for n, p in bb.named_parameters()}
    params = opt.params
    ref = {id(p): [p.detach().cpu().double(), torch.zeros(p.shape, dtype=torch.float64), torch.zeros(p.shape, dtype=torch.float64), p.detach().cpu().double()] for p in params}
    f32 = {id(p): [p.detach().cpu().clone(), torch.zeros(p.shape), torch.zeros(p.shape), p.detach().cpu().clone()] for p in params}
    rows, test = [], "test_product_step_matches_float64_on_its_own_gradients"
    for step in range(1, 5):
        torch.manual_seed(7 + step)
        out = diff.training_step(batch, step)
        out.loss.backward()
        if step == 2:       # foreign gradients: not views of the engine's flat buffer
            for p in params:
                p.grad = p.grad.clone()
        if step == 3:       # one flat parameter sits this step out
            lin_w = {id(l.weight) for l in bb._lins.values()}
            frozen = next(p for p in params if id(p) not in lin_w and p.grad is not None and p.numel() > 1)
            frozen.grad = None
            frozen_before = [t.clone() for t in (frozen.detach(), *opt.state[id(frozen)], opt.ema[id(frozen)])]
        grads = {id(p): p.grad.detach().cpu() for p in params if p.grad is not None}
        assert len(grads) == len(params) - (1 if step == 3 else 0)
        calls.clear()
        opt.step()
        torch.cuda.synchronize()
        # the launches of a step: one multi kernel per kind, never a single-tensor kernel; one pass over the flat gradient buffer for the norm
        assert calls.get("adamw_step_multi") == 1 and calls.get("adamw_step_shadow_multi") == 1, calls
        assert "adamw_step" not in calls and "adamw_step_shadow" not in calls, calls
        assert calls.get("sumsq") == (1 if step in (1, 4) else len(grads)), calls
        # float64 optimizer and fp32 restatement on the same gradients
        gsq = optim_ref.sumsq64(grads.values())
        ed = optim_ref.ema_decay_at(decay, step)
        kw = dict(step=step, gsq=gsq, max_norm=max_norm, ema_decay=ed, **hp)
        for p in params:
            if id(p) not in grads:
                continue
            ref[id(p)] = list(optim_ref.adamw_step64(*ref[id(p)][:1], grads[id(p)], *ref[id(p)][1:3], ref[id(p)][3], **kw))
            pf, mf, vf, ef = f32[id(p)]
            fake_kernels.adamw_step(pf, grads[id(p)], mf, vf, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"], step, torch.tensor(gsq, dtype=torch.float32), max_norm,
                                    ema=ef, ema_decay=ed)
        got = {id(p): (p.detach().cpu(), opt.state[id(p)][0].cpu(), opt.state[id(p)][1].cpu(), opt.ema[id(p)].cpu()) for p in params}
        for qi, q in enumerate(OC.QUANTITIES):
            want = [ref[id(p)][qi] for p in params]
            floor = max(OC.F32_HALF_ULP * OC.max_abs(want), OC.max_dev([f32[id(p)][qi] for p in params], want))
            worst = max(params, key=lambda p: float((got[id(p)][qi].double() - ref[id(p)][qi]).abs().max()))
            rows.append((f"c_large/step{step}/{q}", OC.max_dev([got[id(p)][qi] for p in params], want), OC.BOUND_FACTOR * floor, names[id(worst)]))
        # pre-clip norm: the relative error of the fp32 sum of squares is at most chain * 2^-24 (optim_cases.sumsq_chain), its square root halves it; the per-tensor
        # path adds one fp32 addition per tensor
        n_flat = sum(t.numel() for t in grads.values()) + 64 * len(grads)
        k = OC.sumsq_chain(n_flat) + len(grads)
        rows.append((f"c_large/step{step}/grad_norm_rel", abs(float(opt.grad_norm) - math.sqrt(gsq)) / math.sqrt(gsq), 2 * k * 2.0 ** -24, f"chain {k}"))
        for lin in bb._lins.values():
            assert torch.equal(lin.w16[: lin.out], lin.weight.detach().bfloat16()), f"step {step}: w16 is not the bf16 of its master"
            assert torch.equal(lin.w16t[:, : lin.out], lin.weight.detach().t().bfloat16()), f"step {step}: w16t is not the bf16 of its master"
        if step == 3:
            after = (frozen.detach(), *opt.state[id(frozen)], opt.ema[id(frozen)])
            assert all(torch.equal(a, b) for a, b in zip(after, frozen_before)), f"{names[id(frozen)]} had no gradient but changed"
        opt.zero_grad(set_to_none=True)
    assert opt.step_count == 4 and opt.ema_num_updates == 4
    for key, achieved, bound, where in rows:
        print(f"{test} {key}: achieved {achieved:.3e} bound {bound:.3e} ({where})")
    for key, achieved, bound, where in rows:
        ledger.check(test, key, achieved, bound, note=where)


# ------------------------------------------------------------------------------------------------ job-table layout (csrc/optim.hip: AdamJob / AdamShadowJob)
@pytest.fixture()
def cpu_ptr(monkeypatch):
    """`kernels._p` refuses CPU tensors; the job-table builders only need an address"""
    from unidisc_amd import kernels as K

    monkeypatch.setattr(K, "_p", lambda t: None if t is None else t.data_ptr())
    return K


def test_adamw_job_table_layout(cpu_ptr):
    K = cpu_ptr
    sizes = [1, 1024, 1025, 0, 4099, 3]
    items = []
    for j, n in enumerate(sizes):
        p, g, m, v = (torch.zeros(n) for _ in range(4))
        items.append((p, g, m, v, torch.zeros(n) if j % 2 == 0 else None))
    table, njobs, nchunks = K.adamw_jobs(items, "cpu")
    raw = bytes(table.numpy().tobytes())
    assert table.dtype == torch.uint8 and njobs == len(sizes) and len(raw) == 56 * len(sizes)      # sizeof(AdamJob), static_assert'ed in optim.hip
    chunk0 = 0
    for (p, g, m, v, e), rec in zip(items, struct.iter_unpack("<QQQQQqq", raw)):
        assert rec == (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if e is not None else 0, p.numel(), chunk0)
        chunk0 += math.ceil(p.numel() / 1024)
    assert nchunks == chunk0 == 1 + 1 + 2 + 0 + 5 + 1
    ok = [torch.zeros(8) for _ in range(5)]
    for pos, bad in ((0, torch.zeros(16)[::2]), (1, torch.zeros(8, dtype=torch.float64)), (2, torch.zeros(9)), (3, torch.zeros(8, dtype=torch.bfloat16)), (4, torch.zeros(7))):
        it = list(ok)
        it[pos] = bad
        with pytest.raises(TypeError, match="adamw_jobs " + ("p", "g", "m", "v", "ema")[pos]):
            K.adamw_jobs([tuple(ok), tuple(it)], "cpu")


def test_adamw_shadow_job_table_layout(cpu_ptr):
    K = cpu_ptr
    shapes = [(64, 64), (65, 1), (200, 328), (1, 64)]
    items = []
    for j, (R, C) in enumerate(shapes):
        p, g, m, v = (torch.zeros(R, C) for _ in range(4))
        w16 = torch.zeros(R + 31, C, dtype=torch.bfloat16) if j != 1 else None
        w16t = torch.zeros(C, R + 80, dtype=torch.bfloat16)[:, : R + 17] if j != 2 else None    # a row stride larger than the row
        items.append((p, g, m, v, torch.zeros(R, C) if j % 2 else None, w16, w16t))
    table, njobs, ntiles = K.adamw_shadow_jobs(items, "cpu")
    raw = bytes(table.numpy().tobytes())
    assert njobs == len(shapes) and len(raw) == 88 * len(shapes)        # sizeof(AdamShadowJob)
    tile0 = 0
    for (p, g, m, v, e, w16, w16t), rec in zip(items, struct.iter_unpack("<QQQQQQQqqiiii", raw)):
        R, C = p.shape
        tiles_c = math.ceil(C / 64)
        assert rec == (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if e is not None else 0, w16.data_ptr() if w16 is not None else 0,
                       w16t.data_ptr() if w16t is not None else 0, C if w16 is not None else 0, R + 80 if w16t is not None else 0, R, C, tile0, tiles_c)
        tile0 += math.ceil(R / 64) * tiles_c
    assert ntiles == tile0 == 1 + 2 + 4 * 6 + 1
    R, C = 8, 12
    ok = [torch.zeros(R, C) for _ in range(5)] + [torch.zeros(R, C, dtype=torch.bfloat16), torch.zeros(C, R, dtype=torch.bfloat16)]
    bads = ((0, torch.zeros(C, R).t(), "p"), (1, torch.zeros(R, C, dtype=torch.float64), "g"), (2, torch.zeros(R, C + 1), "m"), (4, torch.zeros(R * C - 1), "ema"),
            (5, torch.zeros(R - 1, C, dtype=torch.bfloat16), "w16"), (6, torch.zeros(C, R - 1, dtype=torch.bfloat16), "w16t"), (5, torch.zeros(R, C), "w16"),
            (6, torch.zeros(R, C, dtype=torch.bfloat16).t(), "w16t"))
    for pos, bad, nm in bads:
        it = list(ok)
        it[pos] = bad
        with pytest.raises(TypeError, match=f"adamw_shadow_jobs {nm}"):
            K.adamw_shadow_jobs([tuple(it)], "cpu")


# ------------------------------------------------------------------------------------------------ the GPU cases must be able to fail
def _wrong_step(variant):
    """optim_ref.adamw_step64 with ONE deliberate mistake, in float64"""
    def step_fn(p, g, m, v, ema, *, lr, betas, eps, weight_decay, step, gsq=None, max_norm=None, ema_decay=0.0):
        p, g, m, v = (t.double() for t in (p, g, m, v))
        b1, b2 = betas
        clip = 1.0
        if max_norm is not None:
            clip = max_norm / (math.sqrt(gsq) + (0.0 if variant == "clip_without_1e-6" else 1e-6))
            if variant != "clip_not_clamped":
                clip = min(1.0, clip)
        g = g * clip
        p_old = p
        if variant == "l2_decay":
            g = g + weight_decay * p
        elif variant != "decay_after_update":
            p = p * (1.0 - lr * weight_decay)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        bc1 = 1.0 if variant == "no_bc1" else 1.0 - b1 ** step
        bc2 = 1.0 if variant == "no_bc2" else 1.0 - b2 ** step
        if variant == "eps_inside_bias_correction":
            denom = (v.sqrt() + eps) / math.sqrt(bc2)
        elif variant == "eps_under_sqrt":
            denom = (v / bc2 + eps).sqrt()
        else:
            denom = v.sqrt() / math.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
        if variant == "decay_after_update":
            p = p * (1.0 - lr * weight_decay)
        e = None
        if ema is not None:
            e = ema.double()
            if variant == "ema_from_old_parameter":
                e = e - (1.0 - ema_decay) * (e - p_old)
            elif variant == "ema_decay_swapped":
                e = e - ema_decay * (e - p)
            else:
                e = e - (1.0 - ema_decay) * (e - p)
        return p, m, v, e
    return step_fn


WRONG_VARIANTS = ("clip_without_1e-6", "clip_not_clamped", "l2_decay", "decay_after_update", "no_bc1", "no_bc2", "eps_inside_bias_correction", "eps_under_sqrt",
                  "ema_from_old_parameter", "ema_decay_swapped")


@pytest.fixture(scope="module")
def teeth_cases():
    return OC.teeth_cases()


def test_wrong_step_without_a_mistake_is_the_reference(teeth_cases):
    case = teeth_cases[1]
    for got, want in zip(case.chain(_wrong_step(None)), case.reference()):
        for q in OC.QUANTITIES:
            assert OC.max_dev(got[q], want[q]) == 0.0


@pytest.mark.parametrize("variant", WRONG_VARIANTS)
def test_optimizer_cases_have_teeth(teeth_cases, variant):
    """Every plausible mistake in the step's arithmetic moves at least one quantity of at least one GPU case (same inputs, same hyper-parameters, same bound:
    tests/optim_cases.py) by more than 10x the bound that case asserts - a kernel with that mistake could not pass tests/test_gpu_optimizer_multi.py."""
    best = (0.0, "")
    for case in teeth_cases:
        for t, (got, want, bound) in enumerate(zip(case.chain(_wrong_step(variant)), case.reference(), case.bounds())):
            for q in OC.QUANTITIES:
                best = max(best, (OC.max_dev(got[q], want[q]) / bound[q], f"{case.name}/step{t + 1}/{q}"))
    print(f"{variant}: {best[0]:.1f} x the asserted bound at {best[1]}")
    assert best[0] > 10.0, f"{variant} stays within 10x the bound of every case (largest: {best[0]:.2f} x at {best[1]})"
