"""Inputs, float64 expectations and bounds of the optimizer-kernel parity cases (tests/test_gpu_optimizer_multi.py), on the CPU.

The GPU tests run the HIP kernels on these inputs; tests/test_optimizer.py::test_optimizer_cases_have_teeth runs deliberately wrong variants of the
arithmetic on the SAME inputs against the SAME bounds - so both import the cases from here.  Nothing in this module touches `unidisc_amd`.

Bound of a compared quantity (p, m, v, ema; per case and step, max-abs over every element of every job):

    floor = max( max|fp32 CPU restatement - fp64 reference| ,  2^-24 * max|fp64 reference| )
    bound = BOUND_FACTOR * floor

The restatement is `fake_kernels.adamw_step` / `adamw_step_shadow` (the same statements in fp32 tensor arithmetic), run as a chain of its own from the same initial
state and gradients; the second term is half an fp32 ulp of the largest value (no fp32 result is closer than that in the worst case; it keeps the floor from
collapsing where the restatement happens to round like the reference on a handful of elements).  Neither term involves a kernel's output.  The kernels differ from
the restatement by contraction (fma), a division where the restatement multiplies, and the host's fp32 rounding of 1 - lr wd, bc1, 1/sqrt(bc2): hence the factor.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import fake_kernels
import optim_ref

BOUND_FACTOR = 5.0      # measured on the MI355X (RESULTS.md "optimizer parity"): the worst row of the ledger sits at 2.23 x its floor; 5 is the smallest round factor with 2x to spare
QUANTITIES = ("p", "m", "v", "ema")
F32_HALF_ULP = 2.0 ** -24


@dataclass
class Hyper:
    lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.01
    max_norm: Optional[float] = None
    gscale: float = 1.0          # gradient magnitude
    gnorm: Optional[float] = None   # rescale every step's gradients to this global norm (the tiny-gradient case)
    step0: int = 1               # number of the first step
    warm: bool = False           # non-zero starting moments
    ema_decay: tuple = (0.9, 0.93, 0.96, 0.99)   # per step


HYPERS = {
    "noclip": Hyper(),
    "clip_active": Hyper(max_norm=1.0, gscale=10.0),                          # norm >> max_norm
    "clip_inactive": Hyper(max_norm=1e5),                                     # norm < max_norm: the coefficient must clamp at 1
    "clip_tiny": Hyper(max_norm=5e-7, gnorm=1e-6),                            # the 1e-6 of the denominator halves the coefficient
    "big_decay": Hyper(lr=0.1, weight_decay=0.2, max_norm=1.0, gscale=10.0),  # lr * wd = 0.02: decay-then-update vs update-then-decay differ by ~2e-3
    "late": Hyper(step0=100000, warm=True, max_norm=1.0, gscale=10.0),        # bias corrections ~ 1 (host double arithmetic), moments in flight
}

SIZES_EDGES = (1, 3, 4, 5, 1023, 1024, 1025, 2048, 4099, 100003)
SHADOW_SHAPES = ((64, 64), (200, 328), (97, 130), (48, 2048), (2048, 512), (1, 64), (65, 1))
SHADOW_PADS = (31, 80, 0, 80, 31, 0, 80)    # extra rows of the shadows: ldt = R + pad is 95, 280, 97, 128, 2079, 1, 145 (both ldt % 8 == 0 and != 0)


def _many_sizes():
    g = torch.Generator().manual_seed(300)
    return tuple(int(x) for x in torch.randint(1, 3000, (300,), generator=g))


@dataclass
class Case:
    name: str
    shapes: tuple                 # per job: (n,) or (R, C)
    hyper: str
    steps: int = 3
    seed: int = 0
    pads: Optional[tuple] = None  # shadow cases: extra shadow rows per job
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def h(self) -> Hyper:
        return HYPERS[self.hyper]

    @property
    def shadow(self):
        return self.pads is not None

    def has_ema(self, j):
        return j % 3 != 1           # EMA for some jobs, null for others in the same table

    def shadow_kinds(self, j):
        """(w16 present, w16t present) of shadow job j"""
        return ((True, True), (True, False), (False, True))[j % 3]

    # ------------------------------------------------------------------ inputs (fp32, CPU, deterministic)
    def inputs(self):
        if "inputs" in self._cache:
            return self._cache["inputs"]
        h = self.h
        gen = torch.Generator().manual_seed(1000 + self.seed)
        p0, m0, v0, e0 = [], [], [], []
        for j, shp in enumerate(self.shapes):
            p0.append(torch.randn(shp, generator=gen) * 2.0)
            m0.append(torch.randn(shp, generator=gen) * (0.1 * h.gscale * 1e-3) if h.warm else torch.zeros(shp))
            v0.append((torch.rand(shp, generator=gen) + 0.01) * (h.gscale * 1e-3) ** 2 if h.warm else torch.zeros(shp))
            e0.append(torch.randn(shp, generator=gen) * 2.0 if self.has_ema(j) else None)
        grads = []
        for t in range(self.steps):
            gs = []
            for shp in self.shapes:
                g = torch.randn(shp, generator=gen) * h.gscale
                if h.gnorm is None:     # a quarter of every gradient ~1e-7: where eps sits in the denominator decides those updates
                    small = torch.rand(shp, generator=gen) < 0.25
                    g = torch.where(small, torch.randn(shp, generator=gen) * 1e-7, g)
                gs.append(g)
            if h.gnorm is not None:
                k = h.gnorm / math.sqrt(optim_ref.sumsq64(gs))
                gs = [(g.double() * k).float() for g in gs]
            grads.append(gs)
        self._cache["inputs"] = (p0, m0, v0, e0, grads)
        return self._cache["inputs"]

    def step_kwargs(self, t, gsq):
        """hyper-parameters of step t (0-based) as keyword arguments of optim_ref.adamw_step64"""
        h = self.h
        return dict(lr=h.lr, betas=h.betas, eps=h.eps, weight_decay=h.weight_decay, step=h.step0 + t, gsq=gsq if h.max_norm is not None else None,
                    max_norm=h.max_norm, ema_decay=h.ema_decay[t])

    def gsq64(self, t):
        return optim_ref.sumsq64(self.inputs()[4][t])

    # ------------------------------------------------------------------ chains
    def chain(self, step_fn):
        """[per step: {quantity: [per job tensor or None]}] of `step_fn(p, g, m, v, ema, **step_kwargs) -> (p, m, v, ema)` applied to every job, its own state
        carried from step to step"""
        p, m, v, e, grads = self.inputs()
        p, m, v, e = list(p), list(m), list(v), list(e)
        out = []
        for t in range(self.steps):
            kw = self.step_kwargs(t, self.gsq64(t))
            for j in range(len(self.shapes)):
                p[j], m[j], v[j], e[j] = step_fn(p[j], grads[t][j], m[j], v[j], e[j], **kw)
            out.append(dict(p=list(p), m=list(m), v=list(v), ema=list(e)))
        return out

    def reference(self):
        if "ref" not in self._cache:
            self._cache["ref"] = self.chain(optim_ref.adamw_step64)
        return self._cache["ref"]

    def restatement(self):
        """the same arithmetic in fp32 on the CPU (fake_kernels), clipping from the fp32 rounding of the float64 sum of squares - what the kernels are given"""
        if "f32" in self._cache:
            return self._cache["f32"]

        def step_fn(p, g, m, v, e, *, lr, betas, eps, weight_decay, step, gsq, max_norm, ema_decay):
            p, m, v = p.clone(), m.clone(), v.clone()
            e = e.clone() if e is not None else None
            gs = torch.tensor(gsq, dtype=torch.float32) if gsq is not None else None
            fake_kernels.adamw_step(p, g, m, v, lr, betas[0], betas[1], eps, weight_decay, step, gs, max_norm, ema=e, ema_decay=ema_decay)
            return p, m, v, e

        self._cache["f32"] = self.chain(step_fn)
        return self._cache["f32"]

    def bounds(self):
        """[per step: {quantity: bound}]"""
        if "bounds" in self._cache:
            return self._cache["bounds"]
        out = []
        for ref, f32 in zip(self.reference(), self.restatement()):
            b = {}
            for q in QUANTITIES:
                floor = F32_HALF_ULP * max_abs(ref[q])
                floor = max(floor, max_dev(f32[q], ref[q]))
                b[q] = BOUND_FACTOR * floor
            out.append(b)
        self._cache["bounds"] = out
        return out


def max_abs(ts):
    return max((float(t.abs().max()) for t in ts if t is not None and t.numel()), default=0.0)


def max_dev(got, ref):
    """max over every element of every job of |got - ref| (float64); a None on one side only is an error"""
    worst = 0.0
    for a, b in zip(got, ref):
        assert (a is None) == (b is None)
        if a is not None and a.numel():
            worst = max(worst, float((a.detach().to("cpu", torch.float64) - b).abs().max()))
    return worst


def flat_cases():
    cs = [Case(f"edges-{h}", tuple((n,) for n in SIZES_EDGES), h, seed=i) for i, h in enumerate(HYPERS)]
    cs.append(Case("many-clip_active", tuple((n,) for n in _many_sizes()), "clip_active", seed=10))    # ~300 jobs: the bisection over chunk0
    cs.append(Case("single-noclip", ((777,),), "noclip", seed=11))
    cs.append(Case("zero_job-clip_active", ((10,), (0,), (2049,), (5,)), "clip_active", seed=12))       # a zero-element job in the middle of the table
    cs.append(Case("gridstride-clip_active", ((5,), (5_000_003,), (1030,)), "clip_active", seed=13))    # 4886 chunks > the 4096-block grid
    return cs


def shadow_cases():
    return [Case(f"shadow-{h}", SHADOW_SHAPES, h, seed=20 + i, pads=SHADOW_PADS) for i, h in enumerate(("clip_active", "late", "big_decay"))]


def teeth_cases():
    """the cases the wrong-variant check runs on the CPU: every hyper-parameter set on the edge sizes, and the 2-D tables (the 5 M-element table adds nothing to it)"""
    return [c for c in flat_cases() if c.name.startswith("edges-")] + shadow_cases()


def sumsq_chain(n):
    """longest chain of fp32 roundings a summand of udm_sumsq_f32 over n elements goes through (csrc/optim.hip): the product, 4 additions per iteration of the
    per-thread loop (3 within the float4, 1 into the running sum), the tail, 6 wave-fold and 3 block-fold additions; then in the final kernel ceil(blocks / 256) loop
    additions, 6 and 3 again.  All summands are non-negative, so the relative error of the result is at most chain * 2^-24 to first order."""
    n4 = n // 4
    grid = max(1, min(1024, (n4 + 255) // 256))
    loop = (n4 + grid * 256 - 1) // (grid * 256)
    return 1 + 4 * loop + 1 + 6 + 3 + (grid + 255) // 256 + 6 + 3
