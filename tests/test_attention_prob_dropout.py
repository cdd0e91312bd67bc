"""Attention-probability dropout (`model.attn_dropout`, reference models/dit.py:1179, :1265 -> sdpa(dropout_p=...) :825-829; shipped in
configs/experiments/jan_cub.yaml) - the CPU side: the mask definition of include/unidisc_hip.h (restated in tests/attn_prob_dropout_ref.py) is a sound
Bernoulli mask, the engine hands every block's forward, backward and recompute the same (p, seed), and the C ABI carries the two new entry points.
The kernels themselves: tests/test_gpu_attention_prob_dropout.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fake_kernels
from attn_prob_dropout_ref import dense_attention, keep_mask, threshold
from golden_utils import Golden
from product_utils import product_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the mask definition
@pytest.mark.parametrize("B,H,L,p,seed", [(4, 2, 320, 0.1, 1234), (4, 3, 200, 0.1, 7), (2, 2, 130, 0.25, (1 << 61) + 5), (1, 16, 1280, 0.1, 99)])
def test_mask_restatement_statistics(B, H, L, p, seed):
    """Drop count within 4 sigma of N thr / 65536 (binomial: sigma^2 = N q (1 - q)); neighbouring keys and neighbouring queries - inside one Philox patch
    or across two - uncorrelated to 4 / sqrt(N) (the standard error of a correlation of N independent pairs is 1 / sqrt(N))."""
    keep = keep_mask(seed, p, B, H, L)
    assert keep.shape == (B, H, L, L)
    N, q = keep.size, threshold(p) / 65536.0
    drop = ~keep
    z = (drop.sum() - N * q) / np.sqrt(N * q * (1 - q))
    ck = np.corrcoef(drop[..., :-1].ravel().astype(np.float64), drop[..., 1:].ravel().astype(np.float64))[0, 1]
    cq = np.corrcoef(drop[..., :-1, :].ravel().astype(np.float64), drop[..., 1:, :].ravel().astype(np.float64))[0, 1]
    print(f"B {B} H {H} L {L} p {p}: z = {z:.2f}, corr_key sqrt(N) = {ck * np.sqrt(N):.2f}, corr_query sqrt(N) = {cq * np.sqrt(N):.2f}")
    assert abs(z) < 4.0, z
    assert abs(ck) < 4.0 / np.sqrt(N) and abs(cq) < 4.0 / np.sqrt(N), (ck, cq, 1 / np.sqrt(N))


def test_mask_depends_on_seed_batch_and_head():
    a = keep_mask(11, 0.1, 2, 2, 130)
    assert not np.array_equal(a, keep_mask(12, 0.1, 2, 2, 130))
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0, 0], a[0, 1])
    assert threshold(0.1) == 6554 and threshold(0.25) == 16384 and threshold(0.0) == 0
    # a patch is 2 queries x 4 keys: rows 2 r, 2 r + 1 and keys 4 g .. 4 g + 3 come from one counter - and differ from each other
    assert not np.array_equal(a[..., 0::2, :][..., :64, :], a[..., 1::2, :][..., :64, :])


# ------------------------------------------------------------------------------------------------ 2. host plumbing with a kernel double
class _Double:
    """fake_kernels with attention_fwd / attention_bwd that take `dropout_p` / `seed` (dense fp32 attention with the restated mask) and record how they
    were called; every other double is fake_kernels' own, wrapped only to note the `seed=` it is given (the residual dropouts)."""

    def __init__(self):
        self.attn, self.other_seeds = [], []
        for name, fn in vars(fake_kernels).items():
            if name.startswith("__"):
                continue
            setattr(self, name, self._noting(name, fn) if callable(fn) and not isinstance(fn, type) else fn)
        self.attention_fwd, self.attention_bwd = self._fwd, self._bwd

    def _noting(self, name, fn):
        def wrapped(*a, **kw):
            if "seed" in kw:
                self.other_seeds.append((name, int(kw["seed"])))
            return fn(*a, **kw)
        return wrapped

    def _dense(self, q, k, v, B, L, H, D, q_prescaled, kw):
        qs = fake_kernels.attention_q_scale(D) if q_prescaled else 1.0
        p, seed = kw.get("dropout_p", 0.0), kw.get("seed", 0)
        keep = keep_mask(int(seed), p, B, H, L) if p else None
        return dense_attention(q / qs, k, v, B, L, H, D, keep=keep, p=p, causal=bool(kw.get("causal", False)))

    def _fwd(self, qkr, qkv, B, L, H, D, sample_ids=None, doc_ranges=None, q_prescaled=False, **kw):
        assert set(kw) <= {"dropout_p", "seed", "causal"}, kw
        self.attn.append(("fwd", dict(kw)))
        if not kw:
            return fake_kernels.attention_fwd(qkr, qkv, B, L, H, D, sample_ids, doc_ranges, q_prescaled)
        assert sample_ids is None and doc_ranges is None
        d = H * D
        return self._dense(qkr[:, :d].float(), qkr[:, d:].float(), qkv[:, 2 * d:].float(), B, L, H, D, q_prescaled, kw).bfloat16(), torch.zeros(B, H, L)

    @torch.enable_grad()
    def _bwd(self, qkr, qkv, o, do, lse, dqkr, dqkv, B, L, H, D, sample_ids=None, doc_ranges=None, q_prescaled=False, **kw):
        assert set(kw) <= {"dropout_p", "seed", "causal"}, kw
        self.attn.append(("bwd", dict(kw)))
        if not kw:
            return fake_kernels.attention_bwd(qkr, qkv, o, do, lse, dqkr, dqkv, B, L, H, D, sample_ids, doc_ranges, q_prescaled)
        d = H * D
        q, k, v = (t.float().clone().requires_grad_() for t in (qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:]))
        self._dense(q, k, v, B, L, H, D, q_prescaled, kw).backward(do.float())
        dqkr[:, :d], dqkr[:, d:], dqkv[:, 2 * d:] = q.grad.bfloat16(), k.grad.bfloat16(), v.grad.bfloat16()


@pytest.fixture
def double(monkeypatch):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod

    fk = _Double()
    monkeypatch.setattr(dit_mod, "K", fk)
    monkeypatch.setattr(diff_mod, "K", fk)
    return fk


def _build(g, attn_dropout, **trainer):
    from unidisc_amd import Diffusion

    cfg = product_config(g.case)
    cfg.model.attn_dropout = attn_dropout
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    diff = Diffusion(cfg, None, "cpu")
    diff.backbone.load_state_dict(g.params(), strict=True)
    diff.backbone.train()
    diff.rng_device = "cpu"
    return diff


def _step(diff, g, backward=True):
    torch.manual_seed(g.case["step_seed"])
    out = diff.training_step(g.batch(), 1)
    if backward:
        out.loss.backward()
    return out


def test_engine_hands_forward_and_backward_the_same_mask(double):
    g = Golden("b_small")
    diff = _build(g, 0.1)          # (the parent raised NotImplementedError here)
    bb = diff.backbone
    n = bb.n_blocks
    assert bb.attn_dropout == pytest.approx(0.1)
    out = _step(diff, g)
    fwd = [kw for kind, kw in double.attn if kind == "fwd"]
    bwd = [kw for kind, kw in double.attn if kind == "bwd"]
    assert len(fwd) == n and len(bwd) == n
    assert all(kw["dropout_p"] == pytest.approx(0.1) for kw in fwd + bwd)
    assert [kw["seed"] for kw in bwd] == [kw["seed"] for kw in fwd][::-1]        # block i's backward regenerates block i's mask
    seeds = [kw["seed"] for kw in fwd]
    assert len(set(seeds)) == n                                                  # another mask in every block ...
    res = {s for _, s in double.other_seeds}
    assert res and not (set(seeds) & res)                                        # ... and none of them a residual dropout's seed
    assert all(s - 2 in res or s - 1 in res for s in seeds)                      # (slot 4 i + 3 beside the block's residual slots 4 i + 1, 4 i + 2)
    loss1 = float(out.loss.detach())
    # a second training forward draws another mask
    double.attn.clear()
    _step(diff, g, backward=False)
    seeds2 = [kw["seed"] for kind, kw in double.attn if kind == "fwd"]
    assert len(seeds2) == n and not (set(seeds2) & set(seeds))
    # another data-parallel rank draws another mask from the same torch seed
    d1 = _build(g, 0.1)
    d1.backbone._dropout_rank = lambda: 1
    double.attn.clear()
    _step(d1, g, backward=False)
    seeds_r1 = [kw["seed"] for kind, kw in double.attn if kind == "fwd"]
    assert len(seeds_r1) == n and not (set(seeds_r1) & set(seeds))
    # the mask is really applied: the same step without attention dropout gives another loss, through calls that carry neither keyword
    d0 = _build(g, None)
    double.attn.clear()
    loss0 = float(_step(d0, g).loss.detach())
    assert double.attn and all(kw == {} for _, kw in double.attn)
    assert loss1 != loss0, (loss1, loss0)   # (a small difference: the golden's attention branches are close to their zero initialisation)


def test_eval_mode_and_no_dropout_call_the_kernels_as_before(double):
    g = Golden("b_small")
    xt, mod = g.t("fp32/xt"), g.t("fp32/modality")
    logits = []
    for p in (0.1, None, 0.0):
        diff = _build(g, p)
        diff.backbone.eval()
        sigma = torch.full((xt.shape[0],), 0.5) if diff.backbone.time_conditioning else None
        double.attn.clear()
        with torch.no_grad():
            logits.append(diff.backbone(xt, sigma, modality=mod))
        assert double.attn and all(kw == {} for _, kw in double.attn)             # neither keyword is passed at all
    assert torch.equal(logits[0], logits[1]) and torch.equal(logits[0], logits[2])


def test_gradient_checkpointing_regenerates_the_same_masks(double):
    g = Golden("b_small")
    res = []
    for ck in (False, True):
        diff = _build(g, 0.1)
        diff.backbone.use_gradient_checkpointing = ck
        double.attn.clear()
        out = _step(diff, g)
        calls = [kw["seed"] for kind, kw in double.attn if kind == "fwd"]
        assert len(calls) == diff.backbone.n_blocks * (2 if ck else 1)            # (the recompute runs the forward kernel again, with the block's seed)
        assert len(set(calls)) == diff.backbone.n_blocks
        res.append((float(out.loss.detach()), {k: p.grad.clone() for k, p in diff.backbone.named_parameters() if p.grad is not None}))
    assert res[0][0] == res[1][0] and set(res[0][1]) == set(res[1][1])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_attention_dropout_refuses_the_masked_paths():
    from unidisc_amd import Diffusion

    g = Golden("b_small")

    def cfg_with(**model):
        cfg = product_config(g.case)
        cfg.model.attn_dropout = 0.1
        for k, v in model.items():
            setattr(cfg.model, k, v)
        return cfg

    cfg = cfg_with()
    cfg.data.require_sample_ids = True
    with pytest.raises(NotImplementedError, match="attn_dropout"):
        Diffusion(cfg, None, "cpu")
    with pytest.raises(NotImplementedError, match="attn_dropout"):
        Diffusion(cfg_with(flex_attention_txt_masking_prob=0.5, flex_attention_img_masking_prob=0.5), None, "cpu")
    with pytest.raises(NotImplementedError, match="attn_dropout"):
        Diffusion(cfg_with(use_attention_mask=True), None, "cpu")
    Diffusion(cfg_with(), None, "cpu")   # alone it builds


# ------------------------------------------------------------------------------------------------ 4. the boundary
def test_dropout_entry_points_are_declared_bound_and_exported():
    from unidisc_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unidisc_hip.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name, base in (("udm_attention_fwd_dropout", "udm_attention_fwd"), ("udm_attention_bwd_dropout", "udm_attention_bwd")):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        assert name in _lib.PROTOTYPES and name in exported and hasattr(lib, name)
        # the old argument list plus (float p_drop, uint64_t seed) in front of the stream
        assert len(params) == len(_lib.PROTOTYPES[name]) == len(_lib.PROTOTYPES[base]) + 2
        assert params[-3].startswith("float ") and params[-2].startswith("uint64_t ") and params[-1].startswith("hipStream_t ")
        assert _lib.PROTOTYPES[name][:-3] == _lib.PROTOTYPES[base][:-1]
        assert _lib.PROTOTYPES[name][-3:] == [_lib._F, _lib._U64, _lib._P]
    assert lib.udm_abi_version() == _lib.ABI_VERSION == 4


def test_kernel_wrappers_route_by_dropout_p(monkeypatch):
    """dropout_p = 0: the old symbols with the old argument tuples; > 0: the `_dropout` symbols with (p, seed) in front of the stream."""
    from unidisc_amd import _lib, kernels as K

    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(K, "_s", lambda: 777)
    monkeypatch.setattr(K, "_p", lambda t: None if t is None else t.data_ptr())   # (host tensors: nothing is launched)
    B, L, H, D = 2, 16, 2, 32
    d = H * D
    q, k, v = (torch.zeros(B * L, d, dtype=torch.bfloat16) for _ in range(3))
    K.attention_fwd_generic(q, k, v, B, L, H, D, causal=True)
    K.attention_fwd_generic(q, k, v, B, L, H, D, causal=True, dropout_p=0.0, seed=5)
    K.attention_fwd_generic(q, k, v, B, L, H, D, causal=True, dropout_p=0.25, seed=5)
    assert [c[0] for c in calls] == ["udm_attention_fwd", "udm_attention_fwd", "udm_attention_fwd_dropout"]
    assert len(calls[0][1]) == len(_lib.PROTOTYPES["udm_attention_fwd"]) and len(calls[2][1]) == len(_lib.PROTOTYPES["udm_attention_fwd_dropout"])
    assert calls[0][1][7:] == calls[1][1][7:] and calls[2][1][-3:] == (0.25, 5, 777) and calls[2][1][7:-3] == calls[0][1][7:-1]
    calls.clear()
    o, lse = torch.zeros_like(q), torch.zeros(B, H, L)
    K.attention_bwd_generic(q, k, v, o, o, lse, B, L, H, D)
    K.attention_bwd_generic(q, k, v, o, o, lse, B, L, H, D, dropout_p=0.1, seed=(1 << 62) + 3)
    assert [c[0] for c in calls] == ["udm_attention_bwd", "udm_attention_bwd_dropout"]
    assert len(calls[0][1]) == len(_lib.PROTOTYPES["udm_attention_bwd"]) and len(calls[1][1]) == len(_lib.PROTOTYPES["udm_attention_bwd_dropout"])
    assert calls[1][1][-3:] == (0.1, (1 << 62) + 3, 777)
