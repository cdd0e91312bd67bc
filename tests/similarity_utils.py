"""Shared by the likelihood-scoring tests: the fixtures of scripts/make_golden_similarity.py (tests/golden/similarity_*.npz), a product configured like the
recorded run, the replay of the recorded uniforms, and the fp64 restatement of the score (model_eval.py:331-370)."""
import os

import numpy as np
import torch

from golden_utils import GOLDEN_DIR, Golden
from product_utils import build_product


class Sim:
    """One recorded top-level call of the reference (`zero_shot_eval_step` or `get_model_likelihood_score`)."""

    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, f"similarity_{name}.npz"))
        self.case_name = str(self.z["meta/case"])
        self.T = int(self.z["meta/T"])
        self.pad = int(self.z["meta/pad_token_id"])
        self.kind = str(self.z["meta/kind"])
        self.guided = bool(self.z["meta/guided"])
        ds = str(self.z["meta/dataset"])
        self.dataset = None if ds == "None" else ds
        self.txt_cond = [bool(v) for v in self.z["meta/txt_cond"]]
        self.do_unconditional = [bool(v) for v in self.z["meta/do_unconditional"]]
        self.n_calls = len(self.txt_cond)
        self.eval_kw = {k[len("meta/eval/"):]: self.z[k].item() for k in self.z.files if k.startswith("meta/eval/")}

    def t(self, key):
        return torch.from_numpy(np.asarray(self.z[key]))

    def has(self, key):
        return key in self.z.files

    def batch(self, device="cpu"):
        return {k[6:]: self.t(k).clone().to(device) for k in self.z.files if k.startswith("batch/")}

    def detailed_calls(self):
        return [c for c in range(self.n_calls) if self.has(f"call{c}/step0/u")]

    def uniforms(self, calls=None):
        calls = range(self.n_calls) if calls is None else calls
        return [self.t(f"call{c}/step{i}/u") for c in calls for i in range(self.T)]

    def product(self, device, **eval_extra):
        """unidisc_amd.Diffusion with the case's parameters, in eval mode, configured like the recorded run (the pad id through eval.pad_token_id)."""
        g = Golden(self.case_name)
        diff = build_product(g, device)
        diff.backbone.eval()
        ev = diff.config.eval
        for k, v in dict(self.eval_kw, pad_token_id=self.pad, **eval_extra).items():
            setattr(ev, k, v)
        if "cfg" not in self.eval_kw:
            ev.cfg = None
        diff.config.data.train = self.dataset
        diff.config.sampling = type(ev)(steps=self.T)
        return diff


def replay_rand(diff, monkeypatch, uniforms):
    """`Diffusion._rand` hands out the recorded draws in order (and refuses any other shape)."""
    queue = list(uniforms)

    def _rand(*shape, device):
        u = queue.pop(0)
        assert tuple(u.shape) == tuple(shape), (tuple(u.shape), shape)
        return u.to(device)

    monkeypatch.setattr(diff, "_rand", _rand)
    return queue


def valid_ids(V, Vt, mask_id, modality_rows, restrict):
    """bool [M, V]: the ids a row's log-sum-exp runs over (model.py:627-635)"""
    M = modality_rows.shape[0]
    v = torch.ones(M, V, dtype=torch.bool)
    if restrict:
        ar = torch.arange(V)[None]
        v = torch.where((modality_rows == 1)[:, None], ar >= Vt, ar < Vt)
    v[:, mask_id] = False
    return v


def loglinear(t, eps=1e-3):
    """(sigma, dsigma) of the log-linear schedule in the precision of t"""
    keep = 1 - eps
    return -torch.log1p(-keep * t), keep / (1 - keep * t)
