"""udm_reveal_rows on a real MI355X (pytest -m gpu): x_out equal to tests/reveal_ref.py BIT FOR BIT for every family of tests/reveal_ref.all_cases, both modes,
B in {1, 3}, every L at which the kernel takes another path (the plan's seams, tests/test_reveal_plan.py) - no row of any case is excluded.  Every operand and
output sits inside a guarded arena (a sentinel id around the int64 buffers, NaN around the fp32 ones, rows padded beyond L): whatever lies outside x_out /
out_noise is compared bit for bit after the launch.  The kernel's own Philox noise is held to a host restatement of its layout."""
import os
import re
import subprocess

import pytest
import torch

import reveal_ref as R
from test_reveal_plan import SEAMS
from tokenchoice_ref64 import GUMBEL_TERM

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = sorted({1, 63, 64, 65, 384, 1280, 4608, 8192} | {s + 1 for s in SEAMS})
GUARD, PAD_COLS, SENTINEL = 64, 3, -(2 ** 62) + 12345


class Arena:
    """device copies of tensors, each inside its own guarded buffer; 2-D tensors get PAD_COLS guard columns per row (a row stride larger than L)"""

    def __init__(self):
        self.bufs = []     # (name, buffer, clone taken before the launch, bool mask of the cells the kernel may write)

    def put(self, name, t, writable=False):
        if t is None:
            return None
        shape = tuple(t.shape)
        rows, cols = (shape[0], shape[1] + PAD_COLS) if t.dim() == 2 else (1, shape[0])
        fill = float("nan") if t.is_floating_point() else (1 if t.dtype == torch.bool else SENTINEL)
        buf = torch.full((GUARD + rows * cols + GUARD,), fill, dtype=t.dtype, device=DEV)
        inner = buf[GUARD:GUARD + rows * cols].view(rows, cols)
        view = inner[:, :shape[1]] if t.dim() == 2 else inner[0]
        view.copy_(t.to(DEV))
        may = torch.zeros_like(buf, dtype=torch.bool)
        if writable:
            m = may[GUARD:GUARD + rows * cols].view(rows, cols)
            (m[:, :shape[1]] if t.dim() == 2 else m[0]).fill_(True)
        self.bufs.append((name, buf, buf.clone(), may))
        return view

    def check(self):
        """everything the kernel may not write is bit for bit what it was"""
        for name, buf, before, may in self.bufs:
            raw = lambda v: v.view(torch.int32) if v.dtype == torch.float32 else (v.view(torch.uint8) if v.dtype == torch.bool else v)
            same = raw(buf) == raw(before)
            assert bool((same | may).all()), f"{name}: {int((~(same | may)).sum())} cells outside the output changed"


def run_kernel(c, *, seed=0, want_noise=False, noise="given"):
    """(x_out, out_noise) on the host from one launch on guarded operands"""
    from unidisc_amd import kernels as K

    B, L = c["x"].shape
    ar = Arena()
    put = lambda k, w=False: ar.put(k, c[k], w)
    out = ar.put("x_out", torch.full((B, L), SENTINEL), True)
    out_noise = ar.put("out_noise", torch.full((B, L), float("nan")), True) if want_noise else None
    got = K.reveal_rows(put("x"), R.MASK, rows=put("rows"), tok=put("tok"), logp=put("logp"), sched=put("sched"), t=put("t"),
                        noise=ar.put("noise", c["noise"] if isinstance(noise, str) else noise), out_noise=out_noise,
                        seed=seed, r_temp=c["r_temp"], lottery=c["lottery"], eos_id=c["eos_id"], pad_id=c["pad_id"], modality=put("modality"), x0=put("x0"),
                        x0_unmask=put("x0_unmask"), out=out)
    torch.cuda.synchronize()
    assert got is out
    ar.check()
    return out.cpu(), (out_noise.cpu() if want_noise else None)


def _kw(c):
    return {k: v for k, v in c.items() if k != "x"}


@pytest.mark.parametrize("lottery", [False, True], ids=["confidence", "lottery"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
def test_x_out_equals_the_rule_bit_for_bit(B, L, lottery):
    cases = R.all_cases(B, L, lottery)
    assert len(cases) >= 50
    for name, c in cases.items():
        want = R.reveal_ref(c["x"], R.MASK, **_kw(c))
        got, _ = run_kernel(c)
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} positions differ"


@pytest.mark.parametrize("lottery", [False, True], ids=["confidence", "lottery"])
def test_pad_only_call(lottery):
    """n = 0 and a schedule of zeros (or none): the EOS rule and the write-back alone - the ddpm_cache path's call"""
    for L in (1, 65, 1280):
        for e in R.EOS_FAMILIES:
            c = R.make_case(3, L, lottery, "random", e, True)
            want = R.reveal_ref(c["x"], R.MASK, **dict(_kw(c), sched=None))
            for sched in (None, torch.zeros(3, dtype=torch.int64)):
                got, _ = run_kernel(dict(c, rows=None, tok=None, logp=None, sched=sched, noise=None, t=c["t"] if sched is not None else None), noise=None)
                assert torch.equal(got, want), (L, e)


@pytest.mark.parametrize("L", [5, 65, 1280, 8192])
def test_philox_noise(L):
    """noise = NULL.  Lottery: out_noise is the host restatement of the layout bit for bit.  Confidence: the Gumbel transform of the same grid points within the
    bound tests/tokenchoice_ref64.py uses for the Philox Gumbel noise of the AR kernel (the same two-branch form).  In both modes a second
    launch with out_noise as explicit noise gives the same x_out bit for bit, x_out is the rule applied to out_noise, and two launches are bit-identical."""
    B, seed = 3, 20240229 + L
    words = R.philox_words(seed, B, L)
    assert bool((R.philox_uniform32(torch.tensor([0, 2 ** 23, 2 ** 24 - 1])) > 0).all()) and float(R.philox_uniform32(torch.tensor([2 ** 24 - 1]))) < 1.0
    for lottery in (False, True):
        for e in (None, "eos_several"):
            c = R.make_case(B, L, lottery, "random", e, True)
            x1, n1 = run_kernel(c, seed=seed, want_noise=True, noise=None)
            x2, n2 = run_kernel(c, seed=seed, want_noise=True, noise=None)
            assert torch.equal(x1, x2) and torch.equal(n1, n2)
            if lottery:
                assert torch.equal(n1, R.philox_uniform32(words))
            else:
                err = (n1.double() - R.philox_gumbel64(words)).abs().max().item()
                print(f"L={L}: worst Gumbel error against fp64 {err:.3e} (bound {GUMBEL_TERM:.1e})")
                assert err <= GUMBEL_TERM
            x3, _ = run_kernel(c, noise=n1)
            assert torch.equal(x3, x1)
            assert torch.equal(x1, R.reveal_ref(c["x"], R.MASK, **dict(_kw(c), noise=n1)))


@pytest.mark.parametrize("lottery", [False, True], ids=["confidence", "lottery"])
def test_malformed_rows_stay_inside_the_operands(lottery):
    """rows out of order, out of range, negative, repeated: wrong tokens are allowed, an access outside the operands is not (the arenas around every operand
    are intact) and every written id is one the operands hold"""
    B, L = 3, 130
    c = R.make_case(B, L, lottery, "random", "eos_several", True)
    n = c["rows"].numel()
    g = torch.Generator().manual_seed(5)
    for kind in ("shuffled", "descending", "out_of_range", "repeated"):
        rows = c["rows"].clone()
        if kind == "shuffled":
            rows = rows[torch.randperm(n, generator=g)]
        elif kind == "descending":
            rows = rows.flip(0)
        elif kind == "out_of_range":
            rows[::3] = torch.tensor([-7, B * L, B * L + 5000, -(2 ** 40), 2 ** 40])[torch.randint(0, 5, (rows[::3].numel(),), generator=g)]
        else:
            rows[:] = rows[n // 2]
        got, _ = run_kernel(dict(c, rows=rows))
        legal = torch.cat([c["x"].reshape(-1), c["tok"], c["x0"].reshape(-1), torch.tensor([R.PAD])]).unique()
        assert bool(torch.isin(got, legal).all()), kind
        keep = c["x"] != R.MASK
        assert bool(((got == c["x"]) | (got == R.PAD) | c["x0_unmask"])[keep].all()), kind     # a revealed token never lands on a position that was not [MASK]


def test_argument_errors():
    from unidisc_amd import kernels as K

    x = torch.full((2, 8193), R.MASK, dtype=torch.int64, device=DEV)
    assert not K.reveal_supported(x)
    with pytest.raises(RuntimeError, match="udm_reveal_rows: L=8193"):
        K.reveal_rows(x, R.MASK)
    x = torch.full((2, 16), R.MASK, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="out of place"):
        K.reveal_rows(x, R.MASK, out=x)
    with pytest.raises(RuntimeError, match="needs t"):
        K.reveal_rows(x, R.MASK, sched=torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="EOS rule"):
        K.reveal_rows(x, R.MASK, eos_id=2)
    with pytest.raises(TypeError, match="int64"):
        K.reveal_rows(x.int(), R.MASK)


def test_symbol_is_exported_with_its_prototype():
    """what tests/test_capi.py asks of every entry point, for this one: declared in the header, bound with the header's arity and float / integer kinds, exported"""
    import ctypes

    from unidisc_amd import _lib

    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unidisc_hip.h")).read(), flags=re.S)
    m = re.search(r"\budm_reveal_rows\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    params = [a.strip() for a in m.group(1).split(",")]
    args = _lib.PROTOTYPES["udm_reveal_rows"]
    assert len(params) == len(args) == 28
    for decl, ct in zip(params, args):
        want = (ctypes.c_float if decl.startswith("float ") else ctypes.c_uint64 if decl.startswith("uint64_t ") else ctypes.c_int if decl.startswith("int ")
                else ctypes.c_int64 if decl.startswith("int64_t ") and "*" not in decl else ctypes.c_void_p)
        assert ct is want, (decl, ct)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "udm_reveal_rows" and " T " in ln for ln in nm.splitlines())
    assert hasattr(lib, "udm_reveal_rows") and lib.udm_abi_version() == _lib.ABI_VERSION == 4
