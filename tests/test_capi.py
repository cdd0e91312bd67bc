"""CPU checks of the C-ABI boundary: the library builds for gfx950, loads, and exports every symbol the header declares."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from unidisc_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    from unidisc_amd import _lib

    header = open(os.path.join(ROOT, "include", "unidisc_hip.h")).read()
    declared = set(re.findall(r"\b(udm_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    bound = set(_lib.PROTOTYPES) | set(_lib.EXTRA_SYMBOLS)
    assert declared == bound, (declared - bound, bound - declared)
    for name in declared:
        assert hasattr(lib, name), name
    # ... and the converse (round 6): the dynamic symbol table holds no `udm_` entry point the header does not declare (diagnostic setters have hidden visibility
    # and are reached through udm_debug_set)
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("udm_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert lib.udm_abi_version() == _lib.ABI_VERSION == 4


def test_prototype_arity_matches_header(lib):
    from unidisc_amd import _lib

    header = open(os.path.join(ROOT, "include", "unidisc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, args in _lib.PROTOTYPES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        n = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n == len(args), (name, n, len(args))


def test_prototype_doubles_match_header(lib):
    """a float bound where the header says double (or the reverse) shifts no argument but passes garbage: the AdamW betas are doubles since ABI 4"""
    import ctypes

    from unidisc_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unidisc_hip.h")).read(), flags=re.S)
    seen = 0
    for name, args in _lib.PROTOTYPES.items():
        params = [a.strip() for a in re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).split(",")]
        for decl, ct in zip(params, args):
            assert (decl.startswith("double ")) == (ct is ctypes.c_double), (name, decl, ct)
            assert (decl.startswith("float ")) == (ct is ctypes.c_float), (name, decl, ct)
            seen += decl.startswith("double ")
    assert seen == 12      # beta1, beta2 of the six udm_adamw_step* entry points


def test_no_cpu_fallback():
    from unidisc_amd import DIT, kernels, make_config, MODEL_PRESETS

    cfg = make_config(**MODEL_PRESETS["tiny"], txt_length=16, img_length=16)
    m = DIT(cfg, 65, 41, 40)
    ids = torch.zeros(2, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(ids, None, modality=torch.zeros_like(ids))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        kernels.gemm_nt(torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16))


def test_state_dict_schema_matches_reference():
    from golden_utils import CASE_NAMES, Golden
    from product_utils import build_product

    for name in CASE_NAMES:
        g = Golden(name)
        diff = build_product(g, "cpu")  # strict load inside
        sd = diff.backbone.state_dict()
        assert set(sd) == set(g.params()), name
        assert all(v.dtype == torch.float32 for v in sd.values())


def test_bench_flops_per_token_match_survey():
    """F_tok = 6 P_mm + 12 n L_att d -> 0.737 (UniDisc-S, L=384), 8.597 (1.4 B, L=1280), 8.522 GFLOP/token (interleaved, L_att=1152)."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert abs(bench.flops_per_token(12, 768, 40193, 384) / 1e9 - 0.737) < 1e-3
    assert abs(bench.flops_per_token(24, 2048, 48385, 1280) / 1e9 - 8.597) < 1e-3
    assert abs(bench.flops_per_token(24, 2048, 48385, 1152) / 1e9 - 8.522) < 1e-3
    for name, w in bench.WORKLOADS.items():   # every workload names a configuration of BASELINE.json
        assert w["desc"] and w["batch"] > 0 and w["txt_length"] + w["img_length"] > 0, name
    b = bench.synthetic_batch("unidisc-1.4b-interleaved-l4608", 2, 0)
    assert b["input_ids"].shape == (2, 4608) and int(b["sample_ids"].max()) == 3 and int((b["modality"] == 1).sum()) == 2 * 4096


def test_bench_kernel_timer_samples_launches(monkeypatch):
    """bench.py brackets 1 GEMM launch in `sample` with events inside the timed region (an event pair per launch costs 1.7 ms per step on the GPU box):
    every call still reaches the library, the pick is reproducible, about 1 / sample of the GEMM launches is recorded and nothing else is."""
    import importlib.util
    import os

    from unidisc_amd import _lib

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class _Ev:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

        def elapsed_time(self, other):
            return 0.25

    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(bench.torch.cuda, "Event", _Ev)
    picks = []
    for _ in range(2):
        calls.clear()
        t = bench.KernelTimer(sample=8)
        t.install()
        t.enabled = True
        for i in range(800):
            _lib.call("udm_gemm_nt_bf16", 0, 0, 0, 64, 64, 64)
            _lib.call("udm_norm_fwd", *([0] * 12))
        t.uninstall()
        assert len(calls) == 1600 and t.seen == 800
        assert 60 <= len(t.records) <= 140 and all(r[2] == "udm_gemm_nt_bf16" for r in t.records)
        s = t.summary()
        assert s["launches"] == len(t.records) and s["launches_seen"] == 800 and abs(s["total_ms"] - 0.25 * len(t.records)) < 1e-9
        assert s["flops"] == 2.0 * 64 ** 3 * len(t.records)
        picks.append(len(t.records))
    assert picks[0] == picks[1]   # seeded: the same launches are bracketed on every run (and on every rank)
    assert _lib.call("x") is None and calls[-1] == "x"   # uninstall restored the plain entry


def test_modality_range_check_on_host_batches_is_immediate():
    """model.py:311: a batch whose `modality` misses a modality (or holds anything but 0 / 1) is refused; on host tensors right away (the deferred form is a
    device-side optimisation, tests/test_gpu_e2e.py)."""
    import pytest as _pytest

    from unidisc_amd.diffusion import Diffusion

    d = Diffusion.__new__(Diffusion)
    d._check_modality_range(torch.tensor([[0, 1, 1], [0, 0, 1]]))
    for bad in (torch.zeros(2, 3, dtype=torch.int64), torch.tensor([[0, 1, 2]]), torch.ones(1, 4, dtype=torch.int64)):
        with _pytest.raises(AssertionError):
            d._check_modality_range(bad)
    assert not d._checks
