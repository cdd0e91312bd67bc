"""The AR baseline (configs/experiments/ar.yaml: parameterization=ar, trainer.ar_shift, model.full_attention=false) for the tests: its config on top of a
golden case's, and the fixtures tests/golden/ar_*.npz (made by scripts/make_golden_ar.py from the imported reference)."""
import os

import numpy as np
import torch

from oracle.cases import CASES
from product_utils import product_config

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AR_CASE_NAMES = ["ar_b_small", "ar_c_large"]


def ar_config(case):
    cfg = product_config(case)
    cfg.parameterization = "ar"
    cfg.trainer.ar_shift = True
    cfg.model.full_attention = False
    return cfg


class ArGolden:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
        self.case = CASES[str(self.z["meta/base_case"])]

    def t(self, key):
        return torch.from_numpy(self.z[key])

    def has(self, key):
        return key in self.z.files

    def params(self):
        return {k[6:]: self.t(k).clone() for k in self.z.files if k.startswith("param/")}

    def grads(self):
        return {k[len("fp32/grad/"):]: self.t(k) for k in self.z.files if k.startswith("fp32/grad/")}

    def grad_floors(self):
        """rel-RMS of the reference's bf16-run gradient against its fp32 one, per parameter"""
        pre = "bf16/grad_relrms/"
        return {k[len(pre):]: float(self.z[k]) for k in self.z.files if k.startswith(pre)}

    def batch(self):
        return {k[6:]: self.t(k).clone() for k in self.z.files if k.startswith("batch/")}


def build_ar_product(golden, device):
    from unidisc_amd import Diffusion

    diff = Diffusion(ar_config(golden.case), None, device)
    diff.backbone.load_state_dict(golden.params(), strict=True)
    diff.backbone.to(device)
    diff.backbone.train()
    return diff
