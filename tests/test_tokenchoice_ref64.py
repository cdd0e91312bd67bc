"""CPU checks of tests/tokenchoice_ref64.py, the fp64 reference the token-choice kernels are held to on the GPU (tests/test_gpu_tokenchoice_rows.py), on that
test's own case list: two independent fp32 emulations of each kernel pass the acceptance rule, every family but `near_tie` leaves no row undecided (all of
`near_tie`'s are), every seeded mutant is rejected on a case this test names, and the host's Philox layouts and Gumbel form hold what the module states."""
import numpy as np
import pytest
import torch

import tokenchoice_ref64 as T

ARITHS = ("torch32", "lanes32")


def _name(shape, family, form):
    return f"V{shape[0]}_mask{shape[2]}/{family}/{form}"


@pytest.mark.parametrize("shape", T.DDPM_SHAPES, ids=lambda s: f"V{s[0]}_mask{s[2]}")
def test_ddpm_emulations_pass_the_rule(shape):
    for sh, family, form in T.ddpm_cases():
        if sh != shape:
            continue
        c, _ = T.ddpm_ref(sh, family, form)
        for arith in ARITHS:
            tok, logp = T.emulate_ddpm(c, form, arith)
            bad, v = T.violations_ddpm(sh, family, form, tok, logp)
            assert bad == [], (_name(sh, family, form), arith, bad)


@pytest.mark.parametrize("shape", T.AR_SHAPES, ids=lambda s: f"V{s[0]}_mask{s[2]}")
def test_ar_emulations_pass_the_rule(shape):
    for sh, family, form in T.ar_cases():
        if sh != shape:
            continue
        c, _ = T.ar_ref(sh, family, form)
        for arith in ARITHS:
            tok, xcol, nid = T.emulate_ar(c, form, arith)
            bad, v = T.violations_ar(sh, family, form, tok, xcol, nid)
            assert bad == [], (_name(sh, family, form), arith, bad)


def test_undecided_counts_are_as_stated():
    """the fp64 reference alone, every case of the GPU test: 0 undecided rows, except near_tie where every row is"""
    for sh, family, form in T.ddpm_cases():
        c, ref = T.ddpm_ref(sh, family, form)
        assert int((~ref.decided).sum()) == (c["M"] if family == "near_tie" else 0), _name(sh, family, form)
    for sh, family, form in T.ar_cases():
        c, ref = T.ar_ref(sh, family, form)
        assert int((~ref.decided).sum()) == (c["M"] if family == "near_tie" else 0), _name(sh, family, form)


def test_families_hold_what_they_promise():
    sh = T.DDPM_SHAPES[3]
    c, ref = T.ddpm_ref(sh, "wave_ties", "race")
    for r in range(c["M"]):
        assert ref.near[r].nonzero()[:, 0].tolist() == c["tied"][r] and int(ref.want[r]) == c["tied"][r][0]
    waves = [sorted({(i % 256) // 64 for i in c["tied"][r]}) for r in range(c["M"])]
    assert [0, 1, 2, 3] in waves[::2] and any(w == [3] for w in waves[3::4])
    assert any((c["tied"][r][0] % 256) // 64 != 0 for r in range(0, c["M"], 2))          # the winner is not always in wave 0
    c, ref = T.ar_ref(T.AR_SHAPES[1], "wave_ties", "g")
    assert any(max(c["tied"][r]) >= 4096 for r in range(c["M"]))                          # a tie that reaches into the second pass
    assert any(len({((i // 8) % 512) // 64 for i in c["tied"][r]}) >= 4 for r in range(0, c["M"], 2))      # (a text row's ids span waves 0 to 4)
    c, ref = T.ddpm_ref(sh, "mask_wins", "race")
    won = ref.want == c["mask_id"]
    assert 20 <= int(won.sum()) <= 44 and bool(ref.zero[3::8].all()) and bool((ref.want[3::8] == 0).all()) and bool(won[7::8].all())
    c, ref = T.ddpm_ref(sh, "u_edges", "race")
    assert bool(((ref.u == 0).sum(-1) >= 1).all()) and bool(((ref.u == 1 - 2.0 ** -24).sum(-1) == 1).all())
    c, ref = T.ddpm_ref(sh, "spikes", "race")
    assert bool((c["valid"].gather(1, ref.want[:, None])[:, 0] | (ref.want == c["mask_id"])).all())      # per row: a valid id or [MASK], never a spiked forbidden id


MUTANT_CASES = {"ddpm": (T.DDPM_MUTANTS, T.ddpm_cases), "ar": (T.AR_MUTANTS, T.ar_cases)}


@pytest.mark.parametrize("kernel,mutant", [(k, m) for k in MUTANT_CASES for m in MUTANT_CASES[k][0]])
def test_rule_rejects_the_mutant(kernel, mutant):
    """every mutant is rejected on at least one case of the GPU test's list; the first such case is printed"""
    for sh, family, form in MUTANT_CASES[kernel][1]():
        if kernel == "ddpm":
            c, _ = T.ddpm_ref(sh, family, form)
            tok, logp = T.emulate_ddpm(c, form, mutant=mutant)
            bad, _ = T.violations_ddpm(sh, family, form, tok, logp)
        else:
            c, _ = T.ar_ref(sh, family, form)
            tok, xcol, nid = T.emulate_ar(c, form, mutant=mutant)
            bad, _ = T.violations_ar(sh, family, form, tok, xcol, nid)
        if bad:
            print(f"{kernel} mutant {mutant}: rejected on {_name(sh, family, form)}: {bad[0]}")
            return
    pytest.fail(f"{kernel} mutant {mutant} passes the rule on every case")


def test_philox_layouts_and_gumbel_form():
    u = T.philox_u_ddpm(5, 3, 1001)
    assert u.dtype == torch.float32 and float(u.min()) >= 0 and float(u.max()) < 1
    w = np.stack(T.philox4x32(5, np.array([2 * 251 + 7], dtype=np.uint64)), -1)[0]       # row 2, ids 28..31: counter row ceil(V / 4) + (id >> 2)
    assert [float(v) for v in u[2, 28:32]] == [float(np.float32((int(x) >> 8) * 2.0 ** -24)) for x in w]
    x = T.philox_x_ar(9, 4, 3, 40)
    key = 9 ^ ((5 * T.GOLDEN) & (2 ** 64 - 1))
    w = np.stack(T.philox4x32(key, np.array([(2 << 40) | 3], dtype=np.uint64)), -1)[0]
    assert x[2, 12:16].tolist() == [int(v) >> 8 for v in w]
    assert not torch.equal(T.philox_x_ar(9, 5, 3, 40), x) and not torch.equal(T.philox_x_ar(10, 4, 3, 40), x)
    # the Gumbel form of the kernel over the grid's ends, its middle and a random sample: finite, and close to fp64 in fp32 terms
    g = torch.Generator().manual_seed(1)
    pts = torch.cat([torch.arange(0, 64), torch.arange(2 ** 23 - 64, 2 ** 23 + 64), torch.arange(2 ** 24 - 64, 2 ** 24), torch.randint(0, 2 ** 24, (4096,), generator=g)])
    g32, g64 = T.gumbel32(pts), T.gumbel64(pts)
    assert bool(torch.isfinite(g32).all())
    assert float((g32.double() - g64).abs().max()) < 4e-6
    top = torch.tensor([2 ** 24 - 1])
    naive = -torch.log(-torch.log(((top.float() + 0.5) * 2.0 ** -24).float()))             # the form before the fix: x + 0.5 rounds to 2^24, u = 1
    assert bool(torch.isinf(naive).all()) and abs(float(T.gumbel64(top)) - 17.3287) < 1e-3
