"""The optimizer kernels a training step actually launches - udm_adamw_step_multi, udm_adamw_step_shadow_multi, udm_sumsq_f32 (csrc/optim.hip) - against a
float64 reference (tests/optim_ref.py) on the inputs and bounds of tests/optim_cases.py.

Every tensor a kernel gets is a 16-byte-aligned slice of a larger buffer filled with a sentinel; the sentinel must be intact after every step, so a tail, tile or
job that runs over its extent fails.  Every element of every tensor is compared (max-abs over the whole table).  The single-tensor entry points run on copies of
the same inputs and must agree with the multi kernels bit for bit (same `adam_update`, same element -> vector / tail path assignment)."""
import pytest
import torch

import ledger
import optim_cases as OC
import optim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.6875       # exactly representable in fp32 and bf16-distinguishable from any N(0, 4) parameter
SENTINEL16 = -1984.0        # exactly representable in bf16


@pytest.fixture(scope="module")
def K():
    from unidisc_amd import kernels
    return kernels


class Packed:
    """CPU tensors (or None) laid out as aligned slices of ONE device buffer with sentinel-filled gaps of at least 16 bytes before, between and after them."""

    def __init__(self, tensors, dtype=torch.float32, sentinel=SENTINEL, align=4, gap=8):
        offs, off = [], gap
        for t in tensors:
            offs.append(off)
            n = t.numel() if t is not None else 0
            off = (off + n + gap + align - 1) // align * align
        host = torch.full((off + gap,), sentinel, dtype=dtype)
        self.written = torch.zeros(off + gap, dtype=torch.bool)      # positions a kernel may write
        self.sentinel = sentinel
        for t, o in zip(tensors, offs):
            if t is not None:
                host[o:o + t.numel()] = t.reshape(-1).to(dtype)
        self.buf = host.to(DEV)
        self.views = [self.buf[o:o + t.numel()].view(t.shape) if t is not None else None for t, o in zip(tensors, offs)]
        self.offs = offs
        for v in self.views:
            assert v is None or v.data_ptr() % 16 == 0

    def allow(self, j, index=None):
        """mark job j's extent (or, 2-D, the rows / columns `index` of it) as writable"""
        v = self.views[j]
        m = self.written[self.offs[j]:self.offs[j] + v.numel()].view(v.shape)
        if index is None:
            m[...] = True
        else:
            m[index] = True

    def load(self, tensors):
        for v, t in zip(self.views, tensors):
            if v is not None:
                v.copy_(t)

    def cpu(self):
        return [v.cpu() if v is not None else None for v in self.views]

    def intact(self):
        return bool((self.buf.cpu()[~self.written] == self.sentinel).all())


def _state(case):
    p0, m0, v0, e0, grads = case.inputs()
    st = dict(p=Packed(p0), m=Packed(m0), v=Packed(v0), ema=Packed(e0), g=Packed(grads[0]))
    for q in ("p", "m", "v", "ema"):
        for j, v in enumerate(st[q].views):
            if v is not None:
                st[q].allow(j)
    return st


def _shadows(case):
    """bf16 shadows of a 2-D case: w16 [R + pad, C], w16t [C, R + pad] (or None per job), sentinel everywhere; only [:R] / [:, :R] may be written"""
    w16, w16t = [], []
    for j, ((R, C), pad) in enumerate(zip(case.shapes, case.pads)):
        has16, has16t = case.shadow_kinds(j)
        w16.append(torch.full((R + pad, C), SENTINEL16) if has16 else None)
        w16t.append(torch.full((C, R + pad), SENTINEL16) if has16t else None)
    a, b = Packed(w16, torch.bfloat16, SENTINEL16, align=8, gap=16), Packed(w16t, torch.bfloat16, SENTINEL16, align=8, gap=16)
    for j, (R, C) in enumerate(case.shapes):
        if a.views[j] is not None:
            a.allow(j, (slice(0, R),))
        if b.views[j] is not None:
            b.allow(j, (slice(None), slice(0, R)))
    return a, b


def _gsq_dev(case, t):
    return torch.tensor([case.gsq64(t)], dtype=torch.float32, device=DEV) if case.h.max_norm is not None else None


def _report_and_check(test, rows):
    """print every achieved error next to its bound (and floor multiple) BEFORE asserting any, then assert all through the ledger"""
    for key, got, bound in rows:
        print(f"{test} {key}: achieved {got:.3e} bound {bound:.3e} = {OC.BOUND_FACTOR:g} x floor; achieved / floor = {got / (bound / OC.BOUND_FACTOR):.2f}")
    for key, got, bound in rows:
        ledger.check(test, key, got, bound, note=f"achieved/floor {got / (bound / OC.BOUND_FACTOR):.2f}")


def _hyper_args(case, t):
    h = case.h
    return (h.lr, h.betas[0], h.betas[1], h.eps, h.weight_decay, h.step0 + t)


@pytest.mark.parametrize("case", OC.flat_cases(), ids=lambda c: c.name)
def test_adamw_step_multi_matches_float64(K, case):
    ref, bounds, grads = case.reference(), case.bounds(), case.inputs()[4]
    multi, single = _state(case), _state(case)
    nj = len(case.shapes)
    items = [(multi["p"].views[j], multi["g"].views[j], multi["m"].views[j], multi["v"].views[j], multi["ema"].views[j]) for j in range(nj)]
    jobs = K.adamw_jobs(items, DEV)      # built once: the pointers do not move between the steps (gradients are copied into place)
    assert jobs[1] == nj and jobs[2] == sum((shp[0] + 1023) // 1024 for shp in case.shapes)
    rows = []
    for t in range(case.steps):
        for st in (multi, single):
            st["g"].load(grads[t])
        gsq, ed = _gsq_dev(case, t), case.h.ema_decay[t]
        K.adamw_step_multi(jobs, *_hyper_args(case, t), gsq, case.h.max_norm, ema_decay=ed)
        for j in range(nj):
            if case.shapes[j][0] > 0:
                K.adamw_step(single["p"].views[j], single["g"].views[j], single["m"].views[j], single["v"].views[j], *_hyper_args(case, t), gsq, case.h.max_norm,
                             ema=single["ema"].views[j], ema_decay=ed)
        torch.cuda.synchronize()
        for q in OC.QUANTITIES:
            got = multi[q].cpu()
            rows.append((f"{case.name}/step{t + 1}/{q}", OC.max_dev(got, ref[t][q]), bounds[t][q]))
            assert multi[q].intact(), f"{case.name} step {t + 1}: the multi kernel wrote outside a job's extent of {q}"
            assert single[q].intact(), f"{case.name} step {t + 1}: the single-tensor kernel wrote outside its tensor ({q})"
            assert torch.equal(multi[q].buf, single[q].buf), f"{case.name} step {t + 1}: {q} of the multi kernel and the single-tensor kernel differ in bits"
        assert torch.equal(torch.cat([g.reshape(-1) for g in multi["g"].cpu()]), torch.cat([g.reshape(-1) for g in grads[t]])), "gradients were modified"
    _report_and_check("test_adamw_step_multi_matches_float64", rows)


@pytest.mark.parametrize("case", OC.shadow_cases(), ids=lambda c: c.name)
def test_adamw_step_shadow_multi_matches_float64(K, case):
    ref, bounds, grads = case.reference(), case.bounds(), case.inputs()[4]
    multi, single = _state(case), _state(case)
    multi["w16"], multi["w16t"] = _shadows(case)
    single["w16"], single["w16t"] = _shadows(case)
    nj = len(case.shapes)
    items = [tuple(multi[q].views[j] for q in ("p", "g", "m", "v", "ema", "w16", "w16t")) for j in range(nj)]
    jobs = K.adamw_shadow_jobs(items, DEV)
    assert jobs[1] == nj and jobs[2] == sum(((R + 63) // 64) * ((C + 63) // 64) for R, C in case.shapes)
    rows = []
    for t in range(case.steps):
        for st in (multi, single):
            st["g"].load(grads[t])
        gsq, ed = _gsq_dev(case, t), case.h.ema_decay[t]
        K.adamw_step_shadow_multi(jobs, *_hyper_args(case, t), gsq, case.h.max_norm, ema_decay=ed)
        for j in range(nj):
            K.adamw_step_shadow(single["p"].views[j], single["g"].views[j], single["m"].views[j], single["v"].views[j], *_hyper_args(case, t), gsq, case.h.max_norm,
                                single["w16"].views[j], single["w16t"].views[j], ema=single["ema"].views[j], ema_decay=ed)
        torch.cuda.synchronize()
        for q in OC.QUANTITIES + ("w16", "w16t"):
            if q in OC.QUANTITIES:
                rows.append((f"{case.name}/step{t + 1}/{q}", OC.max_dev(multi[q].cpu(), ref[t][q]), bounds[t][q]))
            assert multi[q].intact(), f"{case.name} step {t + 1}: the multi kernel wrote outside a job's extent of {q} (padding included)"
            assert single[q].intact(), f"{case.name} step {t + 1}: the single-tensor kernel wrote outside its tensor ({q})"
            assert torch.equal(multi[q].buf, single[q].buf), f"{case.name} step {t + 1}: {q} of the multi kernel and the single-tensor kernel differ in bits"
        # the shadows are the bf16 of the parameter the kernel itself wrote, bit for bit
        for j, (R, C) in enumerate(case.shapes):
            pj = multi["p"].views[j]
            if multi["w16"].views[j] is not None:
                assert torch.equal(multi["w16"].views[j][:R], pj.bfloat16()), f"{case.name} step {t + 1} job {j}: w16 != bf16(p)"
            if multi["w16t"].views[j] is not None:
                assert torch.equal(multi["w16t"].views[j][:, :R], pj.t().bfloat16()), f"{case.name} step {t + 1} job {j}: w16t != bf16(p^T)"
    _report_and_check("test_adamw_step_shadow_multi_matches_float64", rows)


# ------------------------------------------------------------------------------------------------ sum of squares
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2 ** 20, 2 ** 20 + 1, 2 ** 24 + 7, 50_000_000])
def test_sumsq_matches_float64(K, n):
    """All summands are non-negative, so the relative error of the fp32 sum is at most k 2^-24 (1 + O(k 2^-24)) with k the longest chain of roundings; asserted
    against 2 k 2^-24."""
    gen = torch.Generator().manual_seed(n % 1000003)
    x = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 5.0 - 3.0)     # magnitudes 1e-3 .. 1e2
    host = torch.full((n + 16,), 1e30)      # an over-read of the slice would add 1e60 -> inf
    host[8:8 + n] = x
    buf, out = host.to(DEV), torch.full((12,), SENTINEL, device=DEV)
    assert buf[8:8 + n].data_ptr() % 16 == 0 and out[4:5].data_ptr() % 16 == 0
    K.sumsq(buf[8:8 + n], out[4:5])
    torch.cuda.synchronize()
    o = out.cpu()
    assert torch.equal(buf.cpu(), host) and bool((o[:4] == SENTINEL).all()) and bool((o[5:] == SENTINEL).all())
    want = optim_ref.sumsq64([x])
    k = OC.sumsq_chain(n)
    rel = abs(float(o[4].double()) - want) / want
    print(f"sumsq n={n}: k={k} achieved {rel:.3e} bound {2 * k * 2.0 ** -24:.3e}")
    ledger.check("test_sumsq_matches_float64", f"n={n}/rel", rel, 2 * k * 2.0 ** -24, note=f"chain k={k}")


# ------------------------------------------------------------------------------------------------ argument errors (raised on the host: nothing is launched)
def test_multi_entry_points_report_argument_errors(K):
    case = OC.Case("errors", ((64, 64), (5, 8)), "noclip", seed=99, pads=(0, 0))
    st = _state(case)
    st["w16"], st["w16t"] = _shadows(case)
    flat = K.adamw_jobs([tuple(st[q].views[j].reshape(-1) if st[q].views[j] is not None else None for q in ("p", "g", "m", "v", "ema")) for j in range(2)], DEV)
    shadow = K.adamw_shadow_jobs([tuple(st[q].views[j] for q in ("p", "g", "m", "v", "ema", "w16", "w16t")) for j in range(2)], DEV)
    before = {q: st[q].buf.clone() for q in st}
    gsq = torch.ones(1, device=DEV)
    for fn, jobs, name in ((K.adamw_step_multi, flat, "udm_adamw_step_multi"), (K.adamw_step_shadow_multi, shadow, "udm_adamw_step_shadow_multi")):
        with pytest.raises(RuntimeError, match=name + r": bad hyper-parameters \(step 0\)"):
            fn(jobs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0)
        with pytest.raises(RuntimeError, match=name + ": bad hyper-parameters"):
            fn(jobs, 1e-3, 1.0, 0.999, 1e-8, 0.0, 1)
        with pytest.raises(RuntimeError, match=name + ": bad hyper-parameters"):
            fn(jobs, 1e-3, 0.9, 1.5, 1e-8, 0.0, 1)
        with pytest.raises(RuntimeError, match=name + ": clipping needs max_grad_norm > 0"):
            fn(jobs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, gsq, 0.0)
        for bad in (-0.1, 1.5):
            with pytest.raises(RuntimeError, match=name + r": EMA decay must be in \[0, 1\]"):
                fn(jobs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, ema_decay=bad)
        with pytest.raises(RuntimeError, match=name + ": empty"):
            fn((jobs[0], 0, 0), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    torch.cuda.synchronize()
    for q in st:
        assert torch.equal(st[q].buf, before[q]), f"a refused call modified {q}"
