"""The AR baseline at head dim 256 (hidden 512, 2 heads; parameterization = ar, model.full_attention = false, model.use_kv_cache): the KV-cached decode step -
udm_attention_decode at D = 256 - against the full causal forward, with the comparator and bound of test_decode_teacher_forced_matches_full_forward in
tests/test_gpu_ar_sampler.py: every decoded row within 1e-2 rel-RMS of its row of the full forward, and prefill + decode equal to pure decode."""
import pytest
import torch

from ar_utils import ar_config
from golden_utils import rel_err
from oracle.cases import CASES
from test_gpu_ar_sampler import _decode_all

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_decode_matches_full_causal_forward_at_head_dim_256():
    from unidisc_amd import Diffusion

    case = dict(CASES["c_large"], hidden_size=512, n_heads=2, txt_length=40, img_length=64)   # 104 positions: two 64-key splits in the last decode steps
    cfg = ar_config(case)
    cfg.model.use_kv_cache = True
    torch.manual_seed(0)
    diff = Diffusion(cfg, None, DEV)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in sorted(diff.backbone.named_parameters()):
            if n.endswith("linear.weight") or "embed" in n or "attn" in n or "mlp" in n:
                p.copy_((torch.randn(p.shape, generator=gen) * 2 / p.shape[-1] ** 0.5).to(DEV))
    bb = diff.backbone
    bb.eval()
    assert bb.head_dim == 256
    B, L, Vt, V = 3, diff.config.model.length, diff.text_vocab_size, diff.vocab_size
    mod = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    mod[:, diff.static_img_sl] = 1
    x = torch.where(mod == 1, torch.randint(Vt, V, (B, L), generator=gen).to(DEV), torch.randint(0, Vt - 1, (B, L), generator=gen).to(DEV))
    with torch.no_grad():
        full = bb(x, None, modality=mod).float()
        dec = _decode_all(bb, x, mod, 1)
        dec8 = _decode_all(bb, x, mod, 8)
    assert torch.isfinite(full).all() and torch.isfinite(dec).all()
    for p in range(L):
        assert rel_err(dec[:, p], full[:, p]) < 1e-2, p
    assert rel_err(dec8, dec) < 1e-2
    assert bb._kv is None
