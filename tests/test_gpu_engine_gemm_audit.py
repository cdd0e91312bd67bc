"""The engine's own GEMM calls on the GPU (pytest -m gpu) under the auditor of tests/engine_gemm_audit.py: every call of a training step + backward - its operands,
strides, slices, epilogue and schedule as the engine chose them - against the fp64 product within the fp32 summation bounds derived there, with the weight gradients
allocated as NaN and the split-K workspace filled with NaN; then the schedule switches (`multi_wgrads`, `pair_wgrads`, `dgrad_from_w`, `compact_last_block`,
`split_head`), set as attributes of the backbone, compared on inputs that are bit-identical by construction.

Models: d = 256, H = 4, D = 64, two blocks, B = 8 sequences of L = 128, i.e. M = 1024 rows - the smallest shape at which every route exists (`K.gemm_tn_multi` splits
a contraction of at least 16 K tiles of 64 rows).  `plain`: `_PLUMB` of tests/test_gpu_fullwidth_oracle.py without time conditioning; `plain_adaln`: with it (the
adaLN GEMMs and `small_batch_linear_bwd`, no multi route); `mm`: rms + qk-norm + sandwich norms + modality embedding, 64 text + 64 image positions, vocabularies
1001 + 512 under `force_argmax_valid_indices`: the head has 1513 outputs and `split_head` cuts it at the 8-aligned boundaries around the text vocabulary
(`_head_split_cols`: text rows x ids [0, 1008), image rows x ids [1000, 1513) - the slices start at weight row 1000, not 1001: the engine rounds the odd boundary
outwards for alignment).

Every test asserts its dispatch preconditions first and FAILS if the plan stops agreeing.  `gemm_nn_ok(1024, 256, out)` holds for out in (768, 256, 1024), so B = 8
needs no adjustment.  No `_row_split` fires at these shapes with 16 CUs held (every GEMM here has at most 16 tiles; asserted on the CPU in
tests/test_engine_gemm_audit_host.py), so there is no held-CUs case."""
import types

import pytest
import torch

import engine_gemm_audit as E
import ledger
from test_gpu_fullwidth_oracle import _rel
from test_gpu_shadow_lifecycle import forms  # noqa: F401  (the `dgrad_form` spy fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, M = 8, 1024
F64 = torch.float64
BLOCK_LINS = ("qkv", "out", "fc1", "fc2")
BLOCK_WEIGHTS = [(768, 256), (256, 256), (1024, 256), (256, 1024)]          # (out, in) of qkv, out-proj, mlp.0, mlp.2: 3 + 1 + 4 + 4 tiles of 256 x 256
TN = ("gemm_tn", "gemm_tn_splitk", "gemm_tn_pair", "gemm_tn_multi")


def _preconditions():
    from unidisc_amd import kernels as K

    for out in (768, 256, 1024):
        assert K.gemm_nn_ok(M, 256, out), f"gemm_nn_ok({M}, 256, {out}) is False: {M} rows are no longer the nn regime"
    assert all(K.gemm_tn_wants_splitk(o, i) for o, i in BLOCK_WEIGHTS), "a block weight gradient no longer wants split-K: no multi route"
    assert K.gemm_tn_pair_ok(768, 256, 256, M), "qkv + out-proj weight gradients no longer share a launch"
    assert K.GEMM_WS["gemm_tn_multi"](BLOCK_WEIGHTS, M) > 0, f"gemm_tn_multi no longer splits a contraction of {M} rows"
    return K


def _run(model, monkeypatch, test, keep_io=False, **flags):
    """one audited training step + backward of a freshly built, seeded model; every audited call has passed its bound when this returns"""
    K = _preconditions()
    diff = E.build(model, DEV)
    bb = diff.backbone
    for k, v in flags.items():
        assert isinstance(getattr(bb, k), bool), k
        setattr(bb, k, v)
    with E.audit(monkeypatch, K, test, keep_io=keep_io) as aud:
        aud.poison_scratch()
        loss, nlls = E.step(diff, E.batch(model, B))
        calls = aud.resolve(bb)
        gaps = [g.cpu() for g in aud.padding_gaps() if g.numel()]
    grads = {n: p.grad.detach().cpu().clone() for n, p in bb.named_parameters() if p.grad is not None}
    pname = {ln: next(n for n, p in bb.named_parameters() if p is lin.weight) for ln, lin in bb._lins.items()}
    masked = (diff._last["xt"].reshape(-1) == diff.mask_index).cpu()
    return types.SimpleNamespace(aud=aud, calls=calls, gaps=gaps, grads=grads, pname=pname, loss=loss.cpu(), nlls=nlls.cpu(), bb=bb, masked=masked,
                                 split_cols=bb._head_split_cols(), V=bb.vocab_size)


def _wgrad_calls(r, ln):
    return [c for c in r.aud.by(grad=r.pname[ln]) if c.name in TN or (c.name == "gemm_nt" and c.shape[:2] == tuple(r.grads[r.pname[ln]].shape))]


def _route(r, ln):
    return sorted({c.name for c in _wgrad_calls(r, ln)})


def _assert_multi(r, blocks):
    """the four weight gradients of each of `blocks` come from ONE gemm_tn_multi call of four problems over all M rows that returned True; no other multi call"""
    multis = r.aud.by(name="gemm_tn_multi")
    assert len(multis) == len(blocks), [c.shape for c in multis]
    for i in blocks:
        owners = {ln: _wgrad_calls(r, f"{i}.{ln}") for ln in BLOCK_LINS}
        assert all(len(v) == 1 for v in owners.values()), {k: [c.name for c in v] for k, v in owners.items()}
        call = owners["qkv"][0]
        assert all(v[0] is call for v in owners.values()) and call.name == "gemm_tn_multi" and call.result is True, (call.name, call.result)
        assert sorted(call.shape[0]) == sorted(BLOCK_WEIGHTS) and call.shape[1] == M, call.shape
        assert call.launches == ["udm_gemm_tn_multi_bf16"], call.launches


def _assert_healthy(r):
    bad = [n for n, g in r.grads.items() if not bool(torch.isfinite(g).all())]
    assert not bad, f"non-finite gradients (an element of a weight gradient left unwritten?): {bad}"
    assert all(float(g.abs().max()) == 0.0 for g in r.gaps), "an alignment gap of the flat gradient buffer is no longer zero"
    assert all(c.ratios for c in r.calls if c.result is not False), [c.name for c in r.calls if not c.ratios]


def _dgrad_weights(r):
    """{(wrapper, Linear, shadow)} of every call that reads a transposed shadow, or W through gemm_nn"""
    return {(c.name, *c.weight) for c in r.calls if c.weight is not None and (c.weight[1] == "w16t" or c.name.startswith("gemm_nn"))}


# ------------------------------------------------------------------------------------------------ a. the default schedule
@pytest.mark.parametrize("model", ["plain", "plain_adaln", "mm"])
def test_every_engine_gemm_call_is_within_its_fp64_bound(model, monkeypatch):
    r = _run(model, monkeypatch, f"engine_gemm_audit default[{model}]")
    _assert_healthy(r)
    if model == "plain":
        ledger.record("engine_gemm_audit", "fp32 gelu' formula of gelu_tanh_both vs dgelu64, every bf16 in [-12, 12]: 2 x worst |error|", E.dgelu_formula_term())
    table = {ln: _route(r, ln) for ln in r.pname}
    ledger.record(f"engine_gemm_audit default[{model}]", "weight-gradient routes", 0.0, note=str(table))
    if model == "plain_adaln":
        sb = r.aud.by(name="small_batch_linear_bwd")
        assert sorted(g for c in sb for g in c.grads if g.endswith("weight")) == sorted(r.pname[k] for k in ("0.ada", "1.ada", "head.ada")), [c.grads for c in sb]
        assert not r.aud.by(name="gemm_tn_multi"), "adaLN blocks take the multi route"
        return
    # block 0: one shared split-K launch; block 1 (the last): compacted rows through the plain calls
    _assert_multi(r, [0])
    for ln in BLOCK_LINS:
        (c,) = _wgrad_calls(r, f"1.{ln}")
        rows = c.shape[2]
        assert c.name in ("gemm_tn", "gemm_tn_splitk") and ((0 < rows < M) if ln != "qkv" else rows == M), (ln, c.name, c.shape)
    # dgrads: block 0's qkv / out-proj / mlp.0 read W itself, everything else a transposed shadow
    want = {("gemm_nn", f"0.{k}", "w16") for k in ("qkv", "out", "fc1")} | {("gemm_nt", "0.fc2", "w16t")} | {("gemm_nt", f"1.{k}", "w16t") for k in BLOCK_LINS}
    want |= {("gemm_nt_splitk", "head", "w16t")}
    assert _dgrad_weights(r) == want, _dgrad_weights(r) ^ want
    heads = r.aud.by(name="gemm_nt", weight=("head", "w16"))
    if model == "mm":    # (text rows) x ids [0, c_up) and (image rows) x ids [c_al, V)
        c_al, c_up = r.split_cols
        assert (c_al, c_up) == (1000, 1008) and r.V == 1513
        assert sorted((c.c0, c.shape[1]) for c in heads) == [(0, c_up), (c_al, r.V - c_al)], [(c.c0, c.shape) for c in heads]
        assert sorted(c.c0 for c in r.aud.by(name="gemm_nt_splitk", weight=("head", "w16t"))) == [0, c_al]
    else:
        assert [(c.c0, c.shape[1]) for c in heads] == [(0, r.V)]


# ------------------------------------------------------------------------------------------------ b. the weight-gradient schedules
def _wgrad_bound(dy, x):
    """fp32 bound of dW = dY^T X from the captured operands (dY [K, M], X [K, N] bf16)"""
    a, b = dy.to(F64).t(), x.to(F64).t()
    return E.acc_bound(a.abs() @ b.abs().t(), dy.shape[0])


@pytest.mark.parametrize("model", ["plain", "mm"])
def test_wgrad_schedules_agree(model, monkeypatch):
    test = f"engine_gemm_audit wgrad schedules[{model}]"
    runs = [_run(model, monkeypatch, test + " default"), _run(model, monkeypatch, test + " default again"),
            _run(model, monkeypatch, test + " multi off", multi_wgrads=False), _run(model, monkeypatch, test + " multi and pair off", multi_wgrads=False, pair_wgrads=False)]
    for r in runs:
        _assert_healthy(r)
    d0, d1, pair, plain = runs
    # routes of block 0
    _assert_multi(d0, [0]), _assert_multi(d1, [0])
    assert not pair.aud.by(name="gemm_tn_multi") and not plain.aud.by(name="gemm_tn_multi")
    (pc,) = pair.aud.by(name="gemm_tn_pair")
    assert pc.shape == ((768, 256), (256, 256), M) and _wgrad_calls(pair, "0.qkv") == [pc] and _wgrad_calls(pair, "0.out") == [pc], pc.shape
    assert _route(pair, "0.fc1") == ["gemm_tn_splitk"] and _route(pair, "0.fc2") == ["gemm_tn_splitk"]
    assert not plain.aud.by(name="gemm_tn_pair") and all(_route(plain, f"0.{ln}") == ["gemm_tn_splitk"] for ln in BLOCK_LINS)
    # run to run: loss, nlls and every Linear weight gradient reproduce bit for bit; the other tensors are listed
    same = {n: torch.equal(d0.grads[n], d1.grads[n]) for n in d0.grads}
    ledger.record(test, "gradient tensors that do not reproduce bit for bit run to run", sum(not v for v in same.values()), note=str(sorted(n for n, v in same.items() if not v)))
    assert torch.equal(d0.loss, d1.loss) and torch.equal(d0.nlls, d1.nlls)
    lin_w = set(d0.pname.values())
    assert all(same[n] for n in lin_w), sorted(n for n in lin_w if not same[n])
    # across schedules: the weight gradients feed nothing, so everything but block 0's four weight gradients is bit-identical
    blk0 = {d0.pname[f"0.{ln}"] for ln in BLOCK_LINS}
    for r in (pair, plain):
        assert torch.equal(d0.loss, r.loss) and torch.equal(d0.nlls, r.nlls)
        for n in lin_w:
            ops0, ops = d0.aud.operands[n], r.aud.operands[n]
            assert len(ops0) == len(ops) and all(torch.equal(a0, a1) and torch.equal(x0, x1) for (a0, x0), (a1, x1) in zip(ops0, ops)), f"operands of {n} differ"
            if n not in blk0:
                assert torch.equal(d0.grads[n], r.grads[n]), n
    for n in sorted(blk0):
        ((dy, x),) = d0.aud.operands[n]
        bound = 2 * _wgrad_bound(dy, x)
        for what, ra, rb in (("multi vs pair", d0, pair), ("multi vs plain", d0, plain), ("pair vs plain", pair, plain)):
            ledger.check(test, f"{n} {what}: worst |difference| / (2 x fp32 bound)", E.worst_ratio((ra.grads[n].to(F64) - rb.grads[n].to(F64)).abs(), bound), 1.0)


# ------------------------------------------------------------------------------------------------ c. the two dgrad forms
def test_dgrad_forms_agree(forms, monkeypatch):  # noqa: F811
    test = "engine_gemm_audit dgrad forms[plain]"
    nn = _run("plain", monkeypatch, test + " from W", keep_io=True, dgrad_from_w=True)
    nt = _run("plain", monkeypatch, test + " from the transposed shadow", keep_io=True, dgrad_from_w=False)
    _assert_healthy(nn), _assert_healthy(nt)
    assert len(forms) == 2
    in_nn = {f"0.{k}" for k in ("qkv", "out", "fc1")}
    assert all(forms[0][ln] == ("nn" if ln in in_nn else "nt") for ln in nn.pname), forms[0]
    assert all(v == "nt" for v in forms[1].values()), forms[1]
    assert {w[1] for w in _dgrad_weights(nn) if w[0] == "gemm_nn"} == in_nn and not nt.aud.by(name="gemm_nn")
    assert torch.equal(nn.loss, nt.loss)

    def dgrad(r, ln):
        (c,) = [c for c in r.calls if c.weight is not None and c.weight[0] == ln and (c.weight[1] == "w16t" or c.name == "gemm_nn")]
        return c

    # the backward's first dgrad, mlp.2 of block 1, has the same form in both runs: same input, same output.  The first one whose form differs is mlp.0 of block 0:
    # everything above it is the same arithmetic in both runs, so its input is bit-identical, and its two outputs are two roundings of the same product
    a, b = dgrad(nn, "1.fc2"), dgrad(nt, "1.fc2")
    assert a.name == b.name == "gemm_nt" and torch.equal(a.io[0], b.io[0]) and torch.equal(a.io[2], b.io[2])
    a, b = dgrad(nn, "0.fc1"), dgrad(nt, "0.fc1")
    assert (a.name, b.name) == ("gemm_nn", "gemm_nt") and torch.equal(a.io[0], b.io[0]), "the input of block 0's mlp.0 dgrad differs between the two forms"
    assert torch.equal(a.io[1], b.io[1]), "W and its transposed shadow hold different values"
    ref, S, n, _ = E.product_ref(a.io[0].to(F64), a.io[1].to(F64))
    ledger.check(test, "0.fc1 dgrad nn vs nt: worst |difference| / (2 x bf16 bound)",
                 E.worst_ratio((a.io[2].to(F64) - b.io[2].to(F64)).abs(), 2 * E.bf16_bound(ref, E.acc_bound(S, n))), 1.0)


# ------------------------------------------------------------------------------------------------ d. compaction and the head split switched off
def test_compaction_and_head_split_off(monkeypatch):
    test = "engine_gemm_audit compaction and head split[mm]"
    base = _run("mm", monkeypatch, test + " default")
    full = _run("mm", monkeypatch, test + " compact_last_block off", compact_last_block=False)
    whole = _run("mm", monkeypatch, test + " split_head off", split_head=False)
    for r in (base, full, whole):
        _assert_healthy(r)
    _assert_multi(base, [0]), _assert_multi(whole, [0])
    _assert_multi(full, [0, 1])                                      # block 1 on all M rows: the shared launch too
    heads = whole.aud.by(name="gemm_nt", weight=("head", "w16"))
    assert [(c.c0, c.shape[1]) for c in heads] == [(0, whole.V)], [(c.c0, c.shape) for c in heads]
    assert len(base.aud.by(name="gemm_nt", weight=("head", "w16"))) == 2
    # rows outside the masked set: exactly zero in the dY operands of the last block's mlp.2, mlp.0 and out-proj weight gradients (qkv's dY carries dK / dV of every row)
    assert 0 < int(full.masked.sum()) < M and torch.equal(full.masked, base.masked)
    for ln in ("fc2", "fc1", "out"):
        ((dy, x),) = full.aud.operands[full.pname[f"1.{ln}"]]
        assert dy.shape[0] == M and float(dy[~full.masked].abs().max()) == 0.0, f"1.{ln}: a row outside the masked set has a gradient"
        assert float(dy[full.masked].abs().max()) > 0.0
    for what, r in (("compact_last_block off", full), ("split_head off", whole)):
        ledger.record(test, f"{what}: loss and nlls bit-identical to the default run", float(torch.equal(r.loss, base.loss) and torch.equal(r.nlls, base.nlls)))
        ledger.check(test, f"{what}: loss relative difference to the default run", abs(float(r.loss) - float(base.loss)) / abs(float(base.loss)), 5e-5)
        ledger.check(test, f"{what}: nll rel-RMS difference to the default run", _rel(r.nlls, base.nlls), 1e-3)
