"""`bench.py --dump-outputs DIR`: what the timed path handed its caller after its last step, as float32 .npy files.  CPU test of the writer on a
stand-in module (the file set, dtypes, the seeded gradient sample and its reproducibility); GPU test of a plain benchmark run that dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from unidisc_amd.diffusion import Loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _step():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.Linear(64, 8, bias=False))
    m[1].weight.requires_grad_(False)   # a parameter without a gradient is dumped as zeros
    x = torch.randn(4, 96)
    nlls = m(x).float().pow(2)
    loss = nlls.mean()
    loss.backward()
    return m, Loss(loss=loss, img_loss=0, txt_loss=nlls[:, :4].mean().detach(), nlls=nlls.detach(), token_mask=torch.ones(4, 8, dtype=torch.bool))


def test_dump_outputs_files_and_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "GRAD_SAMPLE", 100)
    m, out = _step()
    bench.dump_outputs(str(tmp_path / "a"), out, m)
    bench.dump_outputs(str(tmp_path / "b"), out, m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_norms.npy", "grad_sample.npy", "loss.npy", "nlls.npy", "token_mask.npy", "txt_loss.npy"]   # non-tensor fields are left out
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n   # the same step gives the same files
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(out.loss.item())
    params = list(m.parameters())
    norms = np.load(tmp_path / "a" / "grad_norms.npy")
    assert norms.shape == (3,) and np.allclose(norms[:2], [float(p.grad.norm()) for p in params[:2]]) and norms[2] == 0
    sample = np.load(tmp_path / "a" / "grad_sample.npy")
    assert sample.shape == (100 + 64 + 100,)   # tensors above GRAD_SAMPLE elements are sampled, the 64-element bias whole
    assert np.array_equal(sample[100:164], params[1].grad.numpy()) and not sample[164:].any()
    w = params[0].grad.reshape(-1).numpy()
    assert np.isin(sample[:100], w).all()   # the sample holds gradient elements


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps(tmp_path):
    """A plain run prints the headline fields for exactly --steps timed steps, none of what --full adds, and dumps the last step's outputs."""
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "unidisc-s-l384", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and lines, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["steps"] == 3 and res["unit"] == "tokens/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0 and abs(res["value"] - 64 * 384 / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    assert not {"roofline", "roofline_table", "cpu_baseline"} & set(res)
    files = {n: np.load(d / n) for n in os.listdir(d)}
    assert {"loss.npy", "nlls.npy", "grad_norms.npy", "grad_sample.npy"} <= set(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(d / n) for n in files) < 64 << 20
    assert files["loss.npy"] == np.float32(res["loss"]) and files["nlls.npy"].shape == (64, 384)
