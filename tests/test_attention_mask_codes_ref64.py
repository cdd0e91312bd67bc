"""Attention mask codes on the CPU (the reference side of tests/test_gpu_attention_mask_codes.py).

The sample-id slot of the attention kernels carries mask codes (csrc/attention_common.h: id in the low 32 bits, key class in bits 32-39, query mask in bits 40-47).
Here: (1) the two bf16 flash-attention emulations of tests/attention_ref64.py and the emulated backward stay within the project's row bounds (2u O / dV, 3u dQ / dK,
the lse2 bound) on every code layout the engine builds - the asymmetric modality mask, key padding (class 4), both together, key padding on packed sample ids -
and leave dead rows at lse2 = +inf and exact zeros; (2) the same emulations run with a WRONG predicate are rejected by the same row metric on every layout where the
wrong predicate sees another set of pairs; (3) the key-mask arithmetic the layouts restate is what DIT._attention_masks hands to the attention kernel."""
import pytest
import torch

import attention_ref64 as R
import fake_kernels

B, H, L, D = 4, 2, 320, 64
LAYOUT_CASES = [("modality", 72), ("modality", 128), ("keypad", 72), ("modality_keypad", 72), ("modality_keypad", 128), ("docs_keypad", 72), ("docs_keypad_neg", 72)]
# (b, h, row) entries that see no key, counted by hand: H L for the sample without any attended key; under docs_keypad also H (L // 5 + 1) rows of padding and the
# H x 7 rows of sample 1's first document (positions 0..6), all of whose keys lie in the masked first tile
DEAD_ROWS = dict(keypad=640, docs_keypad=784, docs_keypad_neg=784)


def _dead(codes):
    """(queries that see no key, keys no query sees), each bool [B, H, L]"""
    ok = R.pair_ok(codes)
    return tuple((~ok.any(dim)).unsqueeze(1).expand(B, H, L) for dim in (2, 1))


def _faults(q, k, v, do, ref, codes, prescaled, mutant=None):
    """every miss of a bound or of a dead-row promise, for both forward emulations and the backward from each"""
    dead_q, dead_k = _dead(codes)
    out = []
    for name, fwd in (("oneshot", R.emulate_fwd_oneshot), ("tiled", R.emulate_fwd_tiled)):
        o, lse = fwd(q, k, v, prescaled=prescaled, sample_ids=codes, mutant=mutant)
        dq, dk, dv = R.emulate_bwd(q, k, v, o, do, lse, prescaled=prescaled, sample_ids=codes, mutant=mutant)
        for key, got, dead in (("o", o, dead_q), ("dq", dq, dead_q), ("dk", dk, dead_k), ("dv", dv, dead_k)):
            worst, median, where = R.row_errors(torch.nan_to_num(got, nan=float("inf")), ref[key], ref["sc_" + key])
            if not worst <= R.BOUNDS[key]:
                out.append(f"{name} {key}: worst row {worst / R.U:.2f} u at (b, h, row) = {where}, median {median / R.U:.2f} u")
            if not bool((got[dead] == 0).all()):
                out.append(f"{name} {key}: a dead row is not exactly 0")
        excess, where, dead_ok = R.lse_excess(lse, ref)
        if not (excess <= 1.0 and dead_ok):
            out.append(f"{name} lse2: {excess:.2f} x its bound at {where}, dead rows +inf: {dead_ok}")
    return out


def _case(layout, Lt, family, prescaled):
    codes = R.code_layouts(B, L, Lt)[layout]
    q, k, v, do = R.make_inputs(family, B, H, L, D, prescaled=prescaled, sample_ids=codes, seed=L + D + Lt)
    return codes, (q, k, v, do), R.attention_ref64(q, k, v, do, prescaled=prescaled, sample_ids=codes)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("family", R.FAMILIES_SHORT)
@pytest.mark.parametrize("layout,Lt", LAYOUT_CASES)
def test_emulations_stay_within_the_row_bounds_under_mask_codes(layout, Lt, family, prescaled):
    codes, ops, ref = _case(layout, Lt, family, prescaled)
    dead_q, dead_k = _dead(codes)
    assert torch.equal(torch.isinf(ref["lse2"]), dead_q) and bool((ref["o"][dead_q] == 0).all()) and bool((ref["sc_dk"][dead_k] == 0).all())
    if layout in DEAD_ROWS:
        assert int(dead_q.sum()) == DEAD_ROWS[layout]
    faults = _faults(*ops, ref, codes, prescaled)
    assert not faults, "\n".join(faults)


def test_raw_ids_read_as_before():
    """raw ids (zero high bits) give the id-equality mask; padding is every id < 0"""
    for sid in R.doc_layouts(3, 640).values():
        assert torch.equal(R.pair_ok(sid), (sid[:, :, None] == sid[:, None, :]) & (sid[:, :, None] != -1))
    sid = torch.tensor([[0, 0, -1, -2, -2, 1]])
    assert R.pair_ok(sid)[0].sum() == 5 and not bool(R.pair_ok(sid)[0, 3:5].any())


@pytest.mark.parametrize("mutant", R.PREDICATE_MUTANTS)
def test_a_wrong_predicate_is_rejected(mutant):
    """the emulations with `mutant` in place of attn_pair_ok, judged like the kernels: a miss on EVERY layout whose visibility matrix the mutant changes (Gaussian
    scores: a leaked or lost key carries ordinary weight), and at least one such layout"""
    differs = 0
    for layout, Lt in LAYOUT_CASES:
        codes = R.code_layouts(B, L, Lt)[layout]
        if torch.equal(R.pair_ok(codes, mutant), R.pair_ok(codes)):
            continue
        differs += 1
        codes, ops, ref = _case(layout, Lt, "gauss", True)
        assert _faults(*ops, ref, codes, True, mutant=mutant), f"`{mutant}` passes on {layout} (Lt = {Lt})"
    assert differs >= 1, f"no layout tells `{mutant}` from the predicate"


# ------------------------------------------------------------------------------------------------ the restated key-mask arithmetic is the product's
def _captured_codes(monkeypatch, run):
    from unidisc_amd import dit as dit_mod, diffusion as diff_mod

    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(fake_kernels, name)

        @staticmethod
        def attention_fwd(qkr, qkv, B, L, H, D, sample_ids=None, doc_ranges=None, q_prescaled=False, **kw):
            seen.append((None if sample_ids is None else sample_ids.clone(), doc_ranges))
            return fake_kernels.attention_fwd(qkr, qkv, B, L, H, D, sample_ids, doc_ranges, q_prescaled)

    spy = Spy()
    monkeypatch.setattr(dit_mod, "K", spy)
    monkeypatch.setattr(diff_mod, "K", spy)
    run()
    assert seen and all(torch.equal(s[0], seen[0][0]) for s in seen)       # every block gets the same codes
    return seen[0]


def test_key_mask_codes_are_what_the_engine_hands_to_attention(monkeypatch):
    """the product forward with kernel doubles and an attention_mask, (a) on the packed sample ids of the interleaved golden (tail padding: id -1 under class bits),
    (b) on the modality attention dropout's codes: the sample_ids the attention double receives are key_mask_codes of the same mask, and no doc_ranges go with them"""
    from golden_utils import Golden
    from oracle import unidisc_oracle as O
    from product_utils import build_product
    from unidisc_amd.dit import ModalityMask

    g = Golden("f_interleaved")
    b = O.update_batch(g.cfg, g.batch())
    ids, mod, sid = b["input_ids"], b["modality"], b["sample_ids"]
    nb, n = ids.shape
    assert bool((sid == -1).any()) and int(sid.max()) >= 1
    km = R.key_mask_rows(n)[[0, 2]][:nb]
    diff = build_product(g, "cpu")
    diff.backbone.eval()
    with torch.no_grad():
        codes, ranges = _captured_codes(monkeypatch, lambda: diff.backbone(ids, None, modality=mod, sample_ids=sid, attention_mask=km))
    assert ranges is None and torch.equal(codes, R.key_mask_codes(sid, km))
    assert torch.equal(R.decode_codes(codes)[0], sid) and bool(((codes >> 32) != 0).all())

    g = Golden("g_attn_dropout")
    xt, mod = g.t("fp32/xt"), g.t("fp32/modality")
    nb, n = xt.shape
    Lt = int(g.cfg.txt_length)
    td, idr = torch.arange(nb) % 2 == 1, torch.arange(nb) // 2 % 2 == 1
    km = torch.ones(nb, n, dtype=torch.bool)
    km[0, 1:3], km[-1, Lt - 1:Lt + 2] = False, False
    diff = build_product(g, "cpu")
    diff.backbone.eval()
    with torch.no_grad():
        codes, ranges = _captured_codes(monkeypatch, lambda: diff.backbone(xt, None, modality=mod, attention_mask=km, block_mask=ModalityMask(td, idr, Lt)))
    from unidisc_amd.kernels import modality_mask_codes
    assert ranges is None and torch.equal(codes, R.key_mask_codes(modality_mask_codes(td, idr, Lt, n), km))
