"""The engine's own row-kernel and attention calls on the GPU (pytest -m gpu) under the auditor of tests/engine_rowattn_audit.py: every `norm_fwd`, `norm_bwd`,
`residual_fwd`, `residual_bwd`, `norm_residual_bwd`, `qknorm_rope_fwd`, `qknorm_rope_bwd`, `attention_fwd` and `attention_bwd` call of one training step + backward -
its operands, adaLN chunks, column slices, priors, seeds and mask codes as the engine chose them - against the fp64 restatements of tests/rowops_ref64.py and
tests/attention_ref64.py within the bounds derived there, with the wrappers' workspace filled with NaN; then every backward call is paired with the forward call
whose statistics it was handed.

Models: those of tests/test_gpu_engine_gemm_audit.py (d = 256, H = 4, D = 64, two blocks, B = 8 sequences of L = 128, M = 1024 rows), with every norm weight moved
off 1.  The step seed 125 was chosen on the CPU (the masks are drawn on the CPU generator): it masks 513 .. 576 rows, so that the compacted last block runs on
576 rows - no multiple of L - and, in the masked-attention case, it makes samples that drop text keys, samples that drop image keys and samples that drop
neither; the tests assert both.

Every test first asserts which wrappers and which library entry points were reached: a dispatch change fails the test, it does not audit something else.
`mm_adaln_dropout` is `mm` with `time_conditioning=True`: the only case in which `modality` and `any_img` stand beside an adaLN tensor (modulation and the MLP gate
on the image rows only); `mm` itself has no time conditioning.  At d = 256 the fused adaLN backward (`norm_residual_bwd_ada`, d = 2048 / 4096) does not exist: the adaLN model takes `norm_bwd` + `residual_bwd`.
Left out: a causal (AR) model - `product_config` of tests/product_utils.py passes no `full_attention` key and `make_config` fixes it to True, so no case built
through it reaches `causal=True`; a non-None `doc_ranges` - the engine computes document ranges for packed sample ids only, which none of these models takes,
so the pointer check sees the same `None` in every attention call; `udm_residual_fwd` (no fused next norm) - the engine reaches it only in the checkpointing recompute of an adaLN block."""
import pytest
import torch

import engine_gemm_audit as E
import engine_rowattn_audit as RA
import ledger

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L, M, D_MODEL = 8, 128, 1024, 256
STEP_SEED = 125
MASKING = dict(flex_attention_txt_masking_prob=0.4, flex_attention_img_masking_prob=0.4)
FWD = {"udm_norm_fwd", "udm_qknorm_rope_fwd", "udm_attention_fwd", "udm_residual_norm_fwd"}
BWD_FUSED = {"udm_norm_residual_bwd", "udm_norm_bwd", "udm_attention_bwd", "udm_qknorm_rope_bwd"}
# case -> (model, config keys, backbone attributes, the library entry points the audited calls must launch - and no others)
CASES = {
    "plain": ("plain", None, {}, FWD | BWD_FUSED),
    "plain_adaln": ("plain_adaln", None, {}, (FWD - {"udm_residual_norm_fwd"}) | {"udm_residual_norm_fwd_ada", "udm_norm_bwd", "udm_residual_bwd", "udm_attention_bwd",
                                                                                  "udm_qknorm_rope_bwd"}),
    "mm": ("mm", None, {}, FWD | BWD_FUSED),
    "mm_masking": ("mm", MASKING, {}, FWD | BWD_FUSED),
    "plain_dropout": ("plain", None, dict(dropout=0.1), FWD | BWD_FUSED),
    "plain_adaln_dropout": ("plain_adaln", None, dict(dropout=0.1), (FWD - {"udm_residual_norm_fwd"}) | {"udm_residual_norm_fwd_ada", "udm_norm_bwd", "udm_residual_bwd",
                                                                                                         "udm_attention_bwd", "udm_qknorm_rope_bwd"}),
    # adaLN on a multimodal model: modulation and the MLP gate on the image rows only (`modality`, `any_img` beside the adaLN tensor), sandwich attention branch
    "mm_adaln_dropout": ("mm", dict(time_conditioning=True), dict(dropout=0.1), (FWD - {"udm_residual_norm_fwd"}) | {"udm_residual_norm_fwd_ada", "udm_norm_bwd", "udm_residual_bwd",
                                                                                                                "udm_attention_bwd", "udm_qknorm_rope_bwd"}),
    "plain_attn_dropout": ("plain", None, dict(attn_dropout=0.25), (FWD - {"udm_attention_fwd"}) | (BWD_FUSED - {"udm_attention_bwd"})
                           | {"udm_attention_fwd_dropout", "udm_attention_bwd_dropout"}),
}


def _run(case, monkeypatch):
    from unidisc_amd import kernels as K

    model, cfg, attrs, want_entries = CASES[case]
    test = f"engine_rowattn_audit[{case}]"
    diff = RA.build(model, DEV, case=cfg, **attrs)
    with RA.audit(monkeypatch, K, test) as aud:
        aud.poison_scratch()
        E.step(diff, E.batch(model, B), seed=STEP_SEED)
        aud.pair()
        # ---- dispatch: the wrappers and entry points reached (before any row is judged)
        names = [c.name for c in aud.calls]
        tc = bool(diff.backbone.time_conditioning)
        want = dict(norm_fwd=1, residual_fwd=4, qknorm_rope_fwd=2, attention_fwd=2, attention_bwd=2, qknorm_rope_bwd=2, norm_residual_bwd_ada=0,
                    norm_bwd=5 if tc else 1, residual_bwd=4 if tc else 0, norm_residual_bwd=0 if tc else 4)
        assert {n: names.count(n) for n in want} == want, {n: names.count(n) for n in want}
        assert RA.entries(aud) == want_entries, RA.entries(aud) ^ want_entries
        assert all(len(c.launches) == 1 and not c.inner for c in aud.calls), [(c.name, c.launches, c.inner) for c in aud.calls if len(c.launches) != 1 or c.inner]
    bad = [n for n, p in diff.backbone.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    assert not bad, f"non-finite gradients: {bad}"
    assert all(c.ratios for c in aud.calls)
    ledger.record(test, "audited calls", len(aud.calls), note=f"entry points: {sorted(RA.entries(aud))}; worst ratio per family: "
                  + ", ".join(f"{k} {v:.3f}" for k, v in RA.worst_by_family(aud).items()))
    return aud, diff


def _flags(aud, name):
    return [c.flags for c in aud.by(name)]


def _compacted(aud):
    """row counts of the four residual adds: the last block's two run on the compacted rows"""
    rows = [c.shape[0] for c in aud.by("residual_fwd")]
    assert rows[:2] == [M, M] and rows[2] == rows[3] and 0 < rows[2] < M, rows
    return rows[2]


def test_plain_reaches_the_fused_backward_and_the_compacted_last_block(monkeypatch):
    aud, _ = _run("plain", monkeypatch)
    Mc = _compacted(aud)
    assert Mc % L != 0 and Mc % 64 == 0, f"the compacted last block runs on {Mc} rows: a multiple of L = {L} does not show a row-to-sample map that ignores the compaction"
    # rows_c reached both fused passes of the last block; block 0's run on all rows; the final norm's pass overwrites dx and sums the mlp.2 bias gradient
    fused = [(c.shape[0], c.norm, c.flags) for c in aud.by("norm_residual_bwd")]
    assert fused == [(Mc, "ln", ["acc0", "dbias"]), (Mc, "ln", ["acc1"]), (M, "ln", ["acc1", "dbias"]), (M, "ln", ["acc1"])], fused
    assert aud.S.sid is None and aud.S.p_drop == 0.0 and not aud.draws


def test_plain_adaln_reaches_modulated_norms_both_gates_and_dmod(monkeypatch):
    aud, _ = _run("plain_adaln", monkeypatch)
    assert [c.sig for c in aud.by("norm_fwd")] == [f"norm_fwd ({M}, {D_MODEL}, {L}) ln mod(0, 1)"]
    assert _flags(aud, "residual_fwd") == [["gate2", "next_mod(3, 4)"], ["gate5", "next_mod(0, 1)"]] * 2, _flags(aud, "residual_fwd")
    assert _flags(aud, "norm_bwd") == [["acc0", "mod(0, 1)"], ["acc1", "mod(3, 4)"], ["acc1", "mod(0, 1)"], ["acc1", "mod(3, 4)"], ["acc1", "mod(0, 1)"]], _flags(aud, "norm_bwd")
    assert _flags(aud, "residual_bwd") == [["gate5"], ["gate2"]] * 2 and all(c.norm == "ln" for c in aud.by("norm_bwd"))
    assert all({"dx", "dw", "dshift", "dscale"} <= set(c.ratios) for c in aud.by("norm_bwd")) and all({"dbranch", "dgate"} <= set(c.ratios) for c in aud.by("residual_bwd"))
    assert all(c.shape[0] == M for c in aud.calls if c.name != "attention_fwd" and c.name != "attention_bwd")      # (no compaction with adaLN)


def test_mm_reaches_sandwich_norms_and_the_qk_norm_gradients_in_one_allocation(monkeypatch):
    aud, _ = _run("mm", monkeypatch)
    Mc = _compacted(aud)
    assert all(c.flags == ["w_b", "next"] and c.norm == "rms" for c in aud.by("residual_fwd")), _flags(aud, "residual_fwd")
    assert all({"dw_b", "dw", "dx", "dbranch"} <= set(c.ratios) for c in aud.by("norm_residual_bwd"))
    assert all(f == ["qk_norm1", "q_scale0.1803", "one_allocation"] for f in _flags(aud, "qknorm_rope_bwd")), _flags(aud, "qknorm_rope_bwd")
    assert all({"dgq", "dbq", "dgk", "dbk", "dqk"} <= set(c.ratios) for c in aud.by("qknorm_rope_bwd"))
    assert all({"qkr", "qkr/nr", "stats"} <= set(c.ratios) for c in aud.by("qknorm_rope_fwd"))
    ledger.record("engine_rowattn_audit[mm]", "rows of the compacted last block", Mc)


def test_mm_with_modality_masking_hands_one_set_of_mask_codes_to_every_attention_call(monkeypatch):
    aud, _ = _run("mm_masking", monkeypatch)
    S = aud.S
    assert S.sid is not None and tuple(S.sid.shape) == (B, L)
    qmask = ((S.sid >> 40) & 0xFF).cpu()
    txt, img = qmask[:, 0], qmask[:, -1]                                    # a text query / an image query of every sample: 3 = sees both classes
    kinds = dict(drops_text=int(((txt == 3) & (img == 2)).sum()), drops_images=int(((txt == 1) & (img == 3)).sum()), drops_neither=int(((txt == 3) & (img == 3)).sum()))
    assert all(kinds.values()), f"the step seed no longer covers the three kinds of sample: {kinds}"
    attn = [c for c in aud.calls if c.name.startswith("attention")]
    assert len(attn) == 4 and {c.info["sample_ids"] for c in attn} == {S.sid.data_ptr()}
    # (the engine computes doc ranges for packed sample ids only: under a modality mask every attention call gets the same `None`)
    assert {c.info["doc_ranges"] for c in attn} == {S.doc_ranges.data_ptr() if S.doc_ranges is not None else None}
    assert all(c.flags == ["prescaled1", "causal0", "codes" + ("+ranges" if S.doc_ranges is not None else "")] for c in attn), [c.sig for c in attn]
    ledger.record("engine_rowattn_audit[mm_masking]", "samples per kind", sum(kinds.values()), note=str(kinds))


@pytest.mark.parametrize("case", ["plain_dropout", "plain_adaln_dropout"])
def test_residual_dropout_masks_agree_between_forward_and_backward(case, monkeypatch):
    aud, _ = _run(case, monkeypatch)
    assert aud.S.p_drop == 0.1 and aud.S.p_attn == 0.0
    assert len(aud.draws) == 4 and len({s for _, s in aud.draws}) == 4 and all(c.name == "residual_fwd" for c, _ in aud.draws)
    assert all("drop0.1" in c.flags for n in ("residual_fwd", "residual_bwd", "norm_residual_bwd") for c in aud.by(n))
    if case == "plain_dropout":
        assert _compacted(aud) % L != 0                                    # the mask of the compacted block is drawn on the compacted row index


def test_mm_adaln_reaches_modality_restricted_modulation_and_gate(monkeypatch):
    aud, _ = _run("mm_adaln_dropout", monkeypatch)
    assert int(aud.S.any_img) == 1 and aud.S.modality is not None and aud.S.p_drop == 0.1
    assert [c.flags for c in aud.by("norm_fwd")] == [["mod(0, 1)/img"]] and all(c.norm == "rms" for c in aud.by("norm_fwd") + aud.by("norm_bwd"))
    # the sandwich attention branch: no gate, no dropout; the MLP branch: gate 5 and dropout on the image rows
    assert _flags(aud, "residual_fwd") == [["w_b", "next_mod(3, 4)/img"], ["w_b", "gate5/img", "drop0.1", "next_mod(0, 1)/img"]] * 2, _flags(aud, "residual_fwd")
    assert _flags(aud, "residual_bwd") == [["w_b", "gate5/img", "drop0.1"], ["w_b"]] * 2, _flags(aud, "residual_bwd")
    assert _flags(aud, "norm_bwd") == [["acc0", "mod(0, 1)/img"], ["acc1", "mod(3, 4)/img"], ["acc1", "mod(0, 1)/img"], ["acc1", "mod(3, 4)/img"], ["acc1", "mod(0, 1)/img"]]
    assert all(f[-1] == "one_allocation" for f in _flags(aud, "qknorm_rope_bwd")) and len(aud.draws) == 2
    assert all(c.shape[0] == M for c in aud.calls if not c.name.startswith("attention"))


def test_attention_dropout_masks_agree_between_forward_and_backward(monkeypatch):
    aud, _ = _run("plain_attn_dropout", monkeypatch)
    assert aud.S.p_attn == 0.25 and aud.S.p_drop == 0.0 and aud.S.sid is None
    assert [c.name for c, _ in aud.draws] == ["attention_fwd"] * 2 and len({s for _, s in aud.draws}) == 2
    assert all(c.flags[-1] == "attn_drop0.25" for c in aud.calls if c.name.startswith("attention"))
