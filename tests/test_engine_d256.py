"""Head dim 256 on the host side, with kernel test doubles (tests/fake_kernels.py, as tests/test_engine_orchestration.py): a DIT of hidden size 512 with 2 heads
constructs and runs a training step, and MODEL_PRESETS["xxl"] - the reference's configs/model/xxl.yaml - has head dim 256."""
import pytest
import torch

import fake_kernels
from oracle.cases import CASES
from product_utils import product_config


@pytest.fixture()
def fake_k(monkeypatch):
    import unidisc_amd.dit as dit_mod
    import unidisc_amd.diffusion as diff_mod

    monkeypatch.setattr(dit_mod, "K", fake_kernels)
    monkeypatch.setattr(diff_mod, "K", fake_kernels)
    return fake_kernels


def test_xxl_preset_has_head_dim_256():
    from unidisc_amd.config import MODEL_PRESETS

    xxl = MODEL_PRESETS["xxl"]
    assert xxl == dict(hidden_size=4096, n_heads=16, cond_dim=128, n_blocks=30)
    assert xxl["hidden_size"] // xxl["n_heads"] == 256


def test_dit_with_head_dim_256_constructs_and_steps(fake_k):
    from unidisc_amd import Diffusion

    case = dict(CASES["c_large"], hidden_size=512, n_heads=2, n_blocks=1)
    torch.manual_seed(0)
    diff = Diffusion(product_config(case), None, "cpu")
    bb = diff.backbone
    assert bb.head_dim == 256 and bb.attn_q_scale == fake_k.attention_q_scale(256)
    diff.backbone.train()
    diff.rng_device = "cpu"
    gen = torch.Generator().manual_seed(3)
    B, Lt, Li, Vt = 2, case["txt_length"], case["img_length"], case["text_vocab_size"]
    batch = dict(txt_input_ids=torch.randint(0, Vt - 1, (B, Lt), generator=gen, dtype=torch.int32),
                 img_input_ids=torch.randint(0, case["vocab_size"] - Vt, (B, Li), generator=gen, dtype=torch.int32).to(torch.int16),
                 txt_attention_mask=torch.ones(B, Lt, dtype=torch.bool))
    torch.manual_seed(case["step_seed"])
    out = diff.training_step(batch, 1)
    assert torch.isfinite(out.loss)
    out.loss.backward()
    g = dict(bb.named_parameters())["blocks.0.attention.attn_qkv.weight"].grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_head_dim_512_is_still_refused(fake_k):
    from unidisc_amd import Diffusion

    case = dict(CASES["c_large"], hidden_size=1024, n_heads=2, n_blocks=1)
    with pytest.raises(NotImplementedError, match="32/64/128/256"):
        Diffusion(product_config(case), None, "cpu")
