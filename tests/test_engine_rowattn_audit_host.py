"""The auditor of tests/engine_rowattn_audit.py on the CPU: one training step of the engine on the kernel doubles (tests/fake_kernels.py, fp32 arithmetic with the
kernels' rounding points) stays inside every bound and pairs every backward call with its forward; every mutant - a thin wrapper around ONE double - and both
patches of the engine object are rejected with a message naming the call.

The doubles follow the dispatch of the real wrappers here: `norm_residual_bwd_ada_ok` is the real rule (False at d = 256), so the adaLN model takes `norm_bwd` +
`residual_bwd` as it does on the GPU; one test keeps the doubles' own rule and audits the fused adaLN form."""
import pytest
import torch

import engine_gemm_audit as E
import engine_rowattn_audit as RA
import fake_kernels

TEST = "engine_rowattn_audit_host"
MASKING = dict(flex_attention_txt_masking_prob=0.9, flex_attention_img_masking_prob=0.9)
# model -> (case of engine_gemm_audit.cases(), config keys on top of it, backbone attributes)
MODELS = {"plain": ("plain", None, {}), "plain_adaln": ("plain_adaln", None, {}), "mm": ("mm", None, {}), "mm_masking": ("mm", MASKING, {}),
          "plain_dropout": ("plain", None, dict(dropout=0.1)), "plain_adaln_dropout": ("plain_adaln", None, dict(dropout=0.1)),
          "mm_adaln_dropout": ("mm", dict(time_conditioning=True), dict(dropout=0.1))}   # adaLN on image rows only: modality and any_img beside the adaLN tensor


@pytest.fixture()
def fake_k(monkeypatch):
    import unidisc_amd.dit as dit_mod
    import unidisc_amd.diffusion as diff_mod
    from unidisc_amd import kernels as real

    monkeypatch.setattr(dit_mod, "K", fake_kernels)
    monkeypatch.setattr(diff_mod, "K", fake_kernels)
    monkeypatch.setattr(fake_kernels, "norm_residual_bwd_ada_ok", real.norm_residual_bwd_ada_ok)
    return fake_kernels


def _build(model):
    name, case, attrs = MODELS[model]
    return name, RA.build(name, "cpu", case=case, **attrs)


def _step(model, monkeypatch, test, record=True, prepare=None):
    name, diff = _build(model)
    if prepare is not None:
        prepare(diff.backbone)
    with RA.audit(monkeypatch, fake_kernels, test, record=record) as aud:
        E.step(diff, E.batch(name, 2))
        aud.pair()
    return aud, diff


# ------------------------------------------------------------------------------------------------ the engine on the CPU doubles
@pytest.mark.parametrize("model", sorted(MODELS))
def test_one_fake_kernel_training_step_passes_the_audit(model, fake_k, monkeypatch):
    aud, diff = _step(model, monkeypatch, f"{TEST} {model}")
    bb = diff.backbone
    assert all(torch.isfinite(p.grad).all() for p in bb.parameters() if p.grad is not None)
    assert all(c.ratios and all(r <= 1.0 for r in c.ratios.values()) for c in aud.calls)
    names = [c.name for c in aud.calls]
    tc = "adaln" in model
    # two blocks: norm1 of block 0 on its own, every other norm fused into the residual add in front of it; two attentions
    want = dict(norm_fwd=1, residual_fwd=4, qknorm_rope_fwd=2, attention_fwd=2, attention_bwd=2, qknorm_rope_bwd=2, norm_residual_bwd_ada=0,
                norm_bwd=5 if tc else 1, residual_bwd=4 if tc else 0, norm_residual_bwd=0 if tc else 4)
    assert {n: names.count(n) for n in want} == want
    # the outermost call is audited; what a double runs inside is listed, not counted again
    assert all(c.inner == ["norm_fwd"] for c in aud.by("residual_fwd")) and all(c.inner == ["norm_bwd", "residual_bwd"] for c in aud.by("norm_residual_bwd"))
    S = aud.S
    assert (S.sid is not None) == (model == "mm_masking") and S.p_drop == (0.1 if model.endswith("dropout") else 0.0)
    assert len(aud.draws) == (0 if not model.endswith("dropout") else 2 if model.startswith("mm") else 4)   # (a sandwich attention branch has no dropout)
    if model == "mm_masking":
        qmask = (S.sid >> 40) & 0xFF
        assert bool((qmask != 3).any()), "no sample dropped a modality: the masked attention is not exercised"
        assert {c.info["sample_ids"] for c in aud.calls if c.name.startswith("attention")} == {S.sid.data_ptr()}
    sigs = " | ".join(c.sig for c in aud.calls)
    if model.startswith("plain_adaln"):   # gates 2 and 5, modulation chunks (0, 1) and (3, 4)
        for flag in ("gate2", "gate5", "mod(0, 1)", "mod(3, 4)", "next_mod(3, 4)", "next_mod(0, 1)"):
            assert flag in sigs, flag
    if model == "mm_adaln_dropout":       # modulation and the MLP gate on the image rows only; the sandwich attention branch has no gate
        for flag in ("gate5/img", "mod(0, 1)/img", "mod(3, 4)/img", "next_mod(3, 4)/img", "next_mod(0, 1)/img"):
            assert flag in sigs, flag
        assert "gate2" not in sigs and int(S.any_img) == 1


def test_the_fused_adaln_backward_is_audited_too(monkeypatch):
    """with the doubles' own `norm_residual_bwd_ada_ok` (any whole batch) the adaLN model takes `norm_residual_bwd_ada`: modulated norm + gated branch in one call"""
    import unidisc_amd.dit as dit_mod
    import unidisc_amd.diffusion as diff_mod

    monkeypatch.setattr(dit_mod, "K", fake_kernels)
    monkeypatch.setattr(diff_mod, "K", fake_kernels)
    aud, _ = _step("plain_adaln_dropout", monkeypatch, f"{TEST} fused adaLN form")
    fused = aud.by("norm_residual_bwd_ada")
    # the final norm and the MLP branch below it run apart (the adaLN engine never defers the final norm), block 0's norm1 has nothing below it
    assert len(fused) == 3 and len(aud.by("residual_bwd")) == 1 and len(aud.by("norm_bwd")) == 2
    assert all({"dx", "dbranch", "dw", "dshift", "dscale", "dgate"} <= set(c.ratios) for c in fused)


def test_a_wrapper_the_doubles_do_not_provide_is_reported(fake_k, monkeypatch):
    monkeypatch.delattr(fake_kernels, "qknorm_rope_bwd")
    with pytest.raises(AssertionError, match=r"the engine reached K\.qknorm_rope_bwd, which the kernel doubles do not provide"):
        _step("plain", monkeypatch, TEST + " missing double", record=False)


# ------------------------------------------------------------------------------------------------ mutants: each a thin wrapper around one double
def _rejected(monkeypatch, model, mutants, naming, prepare=None):
    """install the mutants over the doubles, run a step under the auditor, and return the failure, which must name the call"""
    name, diff = _build(model)
    for wrapper, make in mutants.items():
        monkeypatch.setattr(fake_kernels, wrapper, make(getattr(fake_kernels, wrapper), diff.backbone))
    if prepare is not None:
        prepare(diff.backbone)
    with pytest.raises(AssertionError, match=naming) as ei:
        with RA.audit(monkeypatch, fake_kernels, TEST + " mutant", record=False) as aud:
            E.step(diff, E.batch(name, 2))
            aud.pair()
    return str(ei.value)


def test_mutant_gate_chunk_2_read_as_5_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda *a, **kw: real(*a, **dict(kw, gate_idx=5 if kw.get("gate_idx") == 2 else kw.get("gate_idx")))
    _rejected(monkeypatch, "plain_adaln", dict(residual_fwd=m), r"residual_fwd \(256, 256, 128\) ln gate2,next_mod\(3, 4\) x_out")


def test_mutant_shift_and_scale_gradients_swapped_is_rejected(fake_k, monkeypatch):
    def m(real, bb):
        def norm_bwd(*a, **kw):
            if kw.get("dmod") is None:
                return real(*a, **kw)
            d, (i, j), tmp = a[1].shape[1], kw["mod_idx"], torch.zeros_like(kw["dmod"])
            real(*a, **dict(kw, dmod=tmp))
            kw["dmod"][:, i * d:(i + 1) * d] += tmp[:, j * d:(j + 1) * d]
            kw["dmod"][:, j * d:(j + 1) * d] += tmp[:, i * d:(i + 1) * d]
        return norm_bwd
    msg = _rejected(monkeypatch, "plain_adaln", dict(norm_bwd=m), r"norm_bwd \(256, 256, 128\) ln acc1,mod\(3, 4\) dshift")
    assert "mod(3, 4) dscale" in msg and "mod(0, 1) dshift" in msg and " dx:" not in msg       # the input gradient itself is right


def test_mutant_row_to_sample_map_with_L_plus_1_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda x, w, nt, L, **kw: real(x, w, nt, L + 1 if kw.get("mod") is not None else L, **kw)
    msg = _rejected(monkeypatch, "plain_adaln", dict(norm_fwd=m), r"norm_fwd \(256, 256, 128\) ln mod\(0, 1\) y")
    assert "norm_fwd (256, 256, 128) ln mod(0, 1) rstd" not in msg                              # one row of y takes the neighbouring sample's modulation; the statistics are right


def test_mutant_backward_dropout_seed_off_by_one_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda *a, **kw: real(*a, **dict(kw, seed=kw.get("seed", 0) + 1))
    _rejected(monkeypatch, "plain_dropout", dict(residual_bwd=m), r"norm_residual_bwd \(256, 256, 128\) ln acc1,drop0\.1 dbranch")


def test_mutant_q_scale_on_k_as_well_is_rejected(fake_k, monkeypatch):
    def m(real, bb):
        def qk(qkv, *a, **kw):
            out, stats = real(qkv, *a, **kw)
            d = qkv.shape[1] // 3
            out[:, d:] = (out[:, d:].float() * kw.get("q_scale", 1.0)).bfloat16()
            return out, stats
        return qk
    _rejected(monkeypatch, "plain", dict(qknorm_rope_fwd=m), r"qknorm_rope_fwd \(256, 256, 128\) D64 qk_norm0,q_scale0\.1803,rope/L qkr")


def test_mutant_v_read_from_column_d_is_rejected(fake_k, monkeypatch):
    def m(real, bb):
        def attn(qkr, qkv, B, L, H, D, *a, **kw):
            d = H * D
            return real(qkr, torch.cat([qkv[:, :2 * d], qkv[:, d:2 * d]], 1), B, L, H, D, *a, **kw)
        return attn
    msg = _rejected(monkeypatch, "plain", dict(attention_fwd=m), r"attention_fwd \(2, 4, 128, 64\) prescaled1,causal0 o")
    assert "causal0 lse2" not in msg                                                           # the scores do not read v


def test_mutant_accumulate_treated_as_overwrite_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda *a, **kw: real(*a, **dict(kw, accumulate=False))
    msg = _rejected(monkeypatch, "plain", dict(norm_bwd=m), r"norm_bwd \(256, 256, 128\) ln acc1 dx")
    assert "norm_residual_bwd (256, 256, 128) ln acc1 dx" in msg and "acc0,dbias dx" not in msg  # (the double of the fused pass runs the mutant inside)


def test_mutant_attention_bwd_ignoring_sample_ids_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda *a, **kw: real(*a[:11], None, *a[12:], **kw)
    msg = _rejected(monkeypatch, "mm_masking", dict(attention_bwd=m), r"attention_bwd \(2, 4, 128, 64\) prescaled1,causal0,codes dq")
    assert "attention_fwd" not in msg


def test_mutant_next_norm_with_the_wrong_blocks_weight_is_rejected(fake_k, monkeypatch):
    m = lambda real, bb: lambda *a, **kw: real(*a, **dict(kw, next_w=bb.blocks[1].norm2.weight.detach() if kw.get("next_w") is not None else None))
    msg = _rejected(monkeypatch, "plain", dict(residual_fwd=m), r"residual_fwd \(256, 256, 128\) ln next h")
    assert "ln next x_out" not in msg and "ln next rstd_n" not in msg                         # only the weighted output is wrong


# ------------------------------------------------------------------------------------------------ pairing: two patches on the engine object
def test_a_backward_that_receives_another_calls_rstd_is_rejected(fake_k, monkeypatch):
    def prepare(bb):
        forward, kept = bb._block_forward, {}

        def block_forward(S, i, x, pre, **kw):
            x_out, pre_out, R = forward(S, i, x, pre, **kw)
            if i == 0:
                kept["rstd1"] = R.rstd1
            else:
                R.rstd1 = kept["rstd1"]                     # block 1's norm1 backward is handed the statistics of block 0's
            return x_out, pre_out, R
        bb._block_forward = block_forward
    msg = _rejected(monkeypatch, "plain", {}, r"pairing: norm_residual_bwd \(call \d+, norm half\) against norm_fwd \(call 0\): `w` differs", prepare=prepare)
    assert "pairing: norm_fwd (call 0, norm half) has 2 backward partners" in msg and "norm half) has 0 backward partners" in msg


def test_a_dropped_backward_call_is_rejected(fake_k, monkeypatch):
    def prepare(bb):
        bb._norm_backward = lambda bp, pn: bb._finish_block(bp, pn.finish, pn.dmod)              # block 0's norm1 backward never runs
    msg = _rejected(monkeypatch, "plain", {}, r"pairing: norm_fwd \(call 0, norm half\) has 0 backward partners", prepare=prepare)
    assert msg.count("pairing:") == 1


def test_two_dropout_draws_from_one_seed_are_rejected():
    """the engine hands the residual adds of block i the seeds seed0 + 4 i + 1 and + 2, its attention + 3: two recorded draws with one seed fail the pairing"""
    aud = RA.Auditor(fake_kernels, TEST + " seeds", record=False)
    for _ in range(2):
        aud.draws.append((aud._new("residual_fwd", (8, 8, 8), "ln", ["drop0.1"]), 4))
    with pytest.raises(AssertionError, match=r"pairing: residual_fwd \(call 1\) draws its dropout mask from the seed of residual_fwd \(call 0\)"):
        aud.pair(), aud.close()


# ------------------------------------------------------------------------------------------------ pairing: what the engine hands a backward call
def _norm_branch_kw(change):
    """patch `_norm_branch_bwd` of the backbone: `change(kw)` edits the keywords the engine hands the residual-branch backward"""
    def prepare(bb):
        inner = bb._norm_branch_bwd

        def norm_branch_bwd(bp, pn, branch, **kw):
            change(kw)
            return inner(bp, pn, branch, **kw)
        bb._norm_branch_bwd = norm_branch_bwd
    return prepare


def test_a_backward_with_the_other_gate_chunk_is_rejected(fake_k, monkeypatch):
    """the numeric check cannot see this one: the reference of the backward takes the gate the backward was handed"""
    def change(kw):
        if kw.get("gate_idx") == 2:
            kw["gate_idx"] = 5
    msg = _rejected(monkeypatch, "plain_adaln", {}, r"pairing: residual_bwd \(call \d+, resid half\) against residual_fwd \(call \d+\): `gate_idx` differs: forward 2, backward 5",
                    prepare=_norm_branch_kw(change))
    assert msg.count("`gate_idx` differs") == 2 and "exceeds 1" not in msg


def test_a_backward_with_another_seed_is_rejected(fake_k, monkeypatch):
    msg = _rejected(monkeypatch, "plain_adaln_dropout", {}, r"pairing: residual_bwd \(call \d+, resid half\) against residual_fwd \(call \d+\): `seed` differs",
                    prepare=_norm_branch_kw(lambda kw: kw.update(seed=kw["seed"] + 1)))
    assert msg.count("`seed` differs") == 4 and "exceeds 1" not in msg


def test_a_backward_with_another_dropout_probability_is_rejected(fake_k, monkeypatch):
    msg = _rejected(monkeypatch, "plain_dropout", {}, r"pairing: norm_residual_bwd \(call \d+, resid half\) against residual_fwd \(call \d+\): `p_drop` differs: forward 0\.1, backward 0\.2",
                    prepare=_norm_branch_kw(lambda kw: kw.update(p_drop=0.2)))
    assert msg.count("`p_drop` differs") == 4


def test_a_norm_backward_with_the_other_modulation_chunks_is_rejected(fake_k, monkeypatch):
    def prepare(bb):
        inner = bb._norm_backward

        def norm_backward(bp, pn):
            if tuple(pn.mod_idx) == (3, 4):
                pn.mod_idx = (0, 1)
            return inner(bp, pn)
        bb._norm_backward = norm_backward
    msg = _rejected(monkeypatch, "plain_adaln", {}, r"pairing: norm_bwd \(call \d+, norm half\) against residual_fwd \(call \d+\): `mod_idx` differs: forward \(3, 4\), backward \(0, 1\)",
                    prepare=prepare)
    assert msg.count("`mod_idx` differs") == 2


def test_fields_recorded_on_one_side_only_are_reported():
    aud = RA.Auditor(fake_kernels, TEST + " fields", record=False)
    c = aud._new("residual_fwd", (8, 8, 8), "ln", [])
    aud._slot("resid", 1, c, L=8)
    aud._back("resid", 1, aud._new("residual_bwd", (8, 8, 8), None, []), L=8, gate_idx=5)
    with pytest.raises(AssertionError, match=r"the two sides record different fields: \['gate_idx'\]"):
        aud.pair(), aud.close()
