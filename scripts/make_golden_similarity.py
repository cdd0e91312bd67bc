"""Golden vectors of zero-shot likelihood scoring from the IMPORTED reference, CPU fp32, eval mode.  Build container only (the reference does not travel):

    python scripts/make_golden_similarity.py     # writes tests/golden/similarity_*.npz and tests/golden/signatures_similarity.json

TEST INFRASTRUCTURE.  The reference's own `zero_shot_eval_step` (model_eval.py:263-652: its nested `get_similarity` :268-378, the DataComp-style retrieval
branch :567-652 and the Winoground-style branch :479-566) and `get_model_likelihood_score` (:3569-3609) run on oracle/cases.py `b_small` (B = 4, L = 32,
V = 65, 1-D rope) and, for 2-D rope, `c_large`, with T = 4 timesteps.  `get_similarity` is nested and cannot be called from outside, so what happens inside
is captured by wrapping the calls it makes:

  * `q_xt`: x0, the move chance, the `torch.rand(B, L)` draw it makes and x_t.  The checked-out reference unpacks FIVE values from `q_xt`'s SIX
    (model_eval.py:319 against model.py:584): as written the call raises.  The wrapper hands back the first five (it drops `move_indices`, which
    `get_similarity` never uses) - the one accommodation made here; no arithmetic is touched.
  * the noise schedule: t of every timestep;
  * the backbone's forward: the model inputs (conditional, then unconditional under eval.cfg) and the fp32 logits;
  * `torch.stack` of T vectors of B values: the per-timestep weighted, then unweighed, scores of a call;
  * the metric objects (shimmed: `update` records the value) and `rprint` (silenced); `zero_shot_update_batch` (which needs a VAE for Winoground) is
    replaced by its last line (the modality mask): the four Winoground token tensors are synthetic and given.
  * the guidance weight: the reference's `cfg` (:2630-2640) evaluated on (l_c, l_u) = (0, -1), which returns w itself.

Per fixture (one top-level call of the reference): `meta/*` (case, T, pad id, the eval keys, per call txt_cond / do_unconditional), the batch, per call
`call{c}/x0`, `call{c}/weighted` and `/unweighed` [T, B], `call{c}/final` [B], per timestep `call{c}/step{i}/{t, u, xt, inp_cond, inp_uncond, logits_cond,
logits_uncond, w}`, the metric updates and the correctness flags (the reference's comparisons restated on its recorded scores, checked against the
accuracies it reported).  `call{c}/emu_weighted` / `emu_unweighed` are the same scores from the oracle's bf16-emulating forward (oracle/unidisc_oracle.py
`dit_forward(bf16=True)`, the path of test_bf16_emulation_within_reference_noise_floor) on the recorded inputs: their distance from the fp32 scores
(`floor/*`) is the noise floor the GPU test measures the product against.  Fixtures hold arrays only.
"""
from __future__ import annotations

import gc
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle import unidisc_oracle as O  # noqa: E402
from oracle.cases import CASES  # noqa: E402

T = 4
PAD = 7
C = ref_shim.Cfg


class Metric:
    def __init__(self):
        self.values = []

    def update(self, v):
        self.values.append(float(v))

    def compute(self):
        return sum(self.values) / len(self.values) if self.values else float("nan")


METRICS = ["win_text_accuracy", "win_image_accuracy", "win_group_accuracy", "datacomp_img_acc", "datacomp_txt_acc"]


def describe(fn):
    return [dict(name=p.name, kind=p.kind.name, default=None if p.default is inspect.Parameter.empty else repr(p.default),
                 has_default=p.default is not inspect.Parameter.empty) for p in inspect.signature(fn).parameters.values()]


class Tracer:
    """Wraps the calls `get_similarity` / `get_model_likelihood_score` make on the reference object `d`."""

    def __init__(self, d, refeval):
        self.d, self.refeval = d, refeval
        self.qxt, self.fwd, self.ts, self.stacks = [], [], [], []
        self.signature = None
        orig_qxt, orig_bb, orig_noise = d.q_xt, d.backbone.forward, d.noise.forward
        tr = self

        def q_xt(x, move_chance, **kw):
            if tr.signature is None:
                code = sys._getframe(1).f_code
                if code.co_name == "get_similarity":
                    fns = [o for o in gc.get_referrers(code) if inspect.isfunction(o)]
                    tr.signature = describe(fns[0])
            rec = {}
            t_rand = torch.rand

            def rand(*a, **k):
                out = t_rand(*a, **k)
                rec.setdefault("u", out.clone())
                return out

            torch.rand = rand
            try:
                out = orig_qxt(x, move_chance, **kw)
            finally:
                torch.rand = t_rand
            xt = out[0] if isinstance(out, tuple) else out
            tr.qxt.append(dict(x0=x.clone(), move_chance=move_chance.clone(), u=rec["u"], xt=xt.clone()))
            return out[:5] if isinstance(out, tuple) else out     # (see the module docstring: five of the six values)

        def bb_forward(indices, *a, **k):
            out = orig_bb(indices, *a, **k)
            tr.fwd.append(dict(inp=indices.clone(), logits=out.detach().float().clone()))
            return out

        def noise_forward(t):
            tr.ts.append(t.clone())
            return orig_noise(t)

        d.q_xt, d.backbone.forward, d.noise.forward = q_xt, bb_forward, noise_forward
        self._undo = lambda: (setattr(d, "q_xt", orig_qxt), setattr(d.backbone, "forward", orig_bb), setattr(d.noise, "forward", orig_noise))

    def run(self, fn):
        t_stack = torch.stack
        tr = self

        def stack(tensors, *a, **k):
            out = t_stack(tensors, *a, **k)
            if len(tensors) == T and tensors[0].dim() == 1:
                tr.stacks.append(out.clone())
            return out

        torch.stack = stack
        self.refeval.rprint = lambda *a, **k: None
        try:
            with torch.no_grad():
                return fn()
        finally:
            torch.stack = t_stack
            self._undo()


def build(case_name, eval_kw, dataset):
    case = CASES[case_name]
    d = MG.build_reference(case, torch.float32)
    import model_eval as refeval

    d.backbone.eval()
    d.tokenizer = C(pad_token_id=PAD)
    d.config.eval = C(**eval_kw)
    d.config.sampling = C(steps=T)
    d.config.data.train = dataset
    d.zero_shot_update_batch = lambda b: dict(b, modality_mask=torch.nn.functional.one_hot(b["modality"], num_classes=2).to(torch.bool))   # model.py:154
    for m in METRICS:
        d.__dict__[m] = Metric()
    return d, case, refeval


def retrieval_batch(d, case):
    b = d.update_batch({k: v.clone() for k, v in MG.make_batch(case).items()})
    b["input_ids"] = torch.where(b["attention_mask"], b["input_ids"], torch.full_like(b["input_ids"], PAD))   # padding holds the pad id
    return b


def wino_batch(d, case):
    b = retrieval_batch(d, case)
    g = torch.Generator().manual_seed(4242)
    B, Lt, Li, Vt, V = case["batch_size"], case["txt_length"], case["img_length"], case["text_vocab_size"], case["vocab_size"]
    cap = [torch.randint(0, Vt - 1, (B, Lt), generator=g) for _ in range(2)]
    img = [torch.randint(Vt, V, (B, Li), generator=g) for _ in range(2)]
    cap[0][1, Lt - 3:] = PAD
    cap[1][2, Lt - 5:] = PAD
    for i in (0, 1):
        for j in (0, 1):
            b[f"input_ids_{i}_{j}"] = torch.cat([cap[i], img[j]], -1)
    return b


def oracle_scores(case_name, params, call, steps, guided, do_unconditional, cond_mask, valid, modality, bf16):
    """The reference's tensor statements (model_eval.py:331-370) on logits of the oracle's forward of the recorded inputs -> (weighted, unweighed) [T, B]."""
    cfg = O.OracleConfig.from_case(CASES[case_name])
    bufs = buffers_of(case_name)
    ws, us = [], []
    for st in steps:
        lc = O.dit_forward(cfg, params, bufs, st["inp_cond"], None, modality, bf16=bf16)
        if guided:
            lu = O.dit_forward(cfg, params, bufs, st["inp_uncond"], None, modality, bf16=bf16)
            w = st["w"].reshape(-1, 1, 1)
            lc = (1 + w) * lc - w * lu
        lp = O.subs_parameterization(cfg, lc.float(), st["xt"], modality, dict(modality=modality), bf16=False)
        log_p = torch.gather(lp, -1, call["x0"][:, :, None]).squeeze(-1)
        log_p = torch.where(valid, log_p, torch.zeros_like(log_p))
        if cond_mask is not None and not do_unconditional:
            log_p = torch.where(cond_mask, torch.zeros_like(log_p), log_p)
        sigma, dsigma = O.loglinear_noise(st["t"])
        ws.append((-log_p * (dsigma / torch.expm1(sigma))[:, None]).sum(-1) / valid.sum(-1))
        us.append((-log_p).sum(-1) / valid.sum(-1))
    return torch.stack(ws), torch.stack(us)


def buffers_of(case_name):
    """rotary tables of the case (the ones tests/golden/<case>.npz already holds)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from golden_utils import Golden

    return Golden(case_name).buffers()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def record(name, case_name, eval_kw, dataset, kind, call_specs, detail_calls=None, seed=2024):
    """kind: "zero_shot" or "likelihood"; call_specs: per get_similarity call in the order the branch makes them, (txt_cond, do_unconditional);
    detail_calls: the calls whose per-timestep records are written (None: all) - every call's scores are."""
    d, case, refeval = build(case_name, eval_kw, dataset)
    batch = wino_batch(d, case) if dataset == "facebook/winoground" else retrieval_batch(d, case)
    tr = Tracer(d, refeval)
    torch.manual_seed(seed)
    ret = {}
    if kind == "zero_shot":
        tr.run(lambda: d.zero_shot_eval_step(batch, 0))
    else:
        ret["final"] = tr.run(lambda: d.get_model_likelihood_score(batch, num_timesteps=T, **eval_kw.get("_kw", {})))
    guided = eval_kw.get("cfg") is not None and kind == "zero_shot"
    n_calls = len(call_specs)
    per = 2 if guided else 1
    assert len(tr.qxt) == n_calls * T and len(tr.fwd) == n_calls * T * per and len(tr.ts) == n_calls * T and len(tr.stacks) == 2 * n_calls, \
        (len(tr.qxt), len(tr.fwd), len(tr.ts), len(tr.stacks))
    modality = batch["modality"]
    Lt = case["txt_length"]
    params = {n: p.detach().clone() for n, p in d.backbone.named_parameters()}
    out = {"meta/case": np.array(case_name), "meta/T": np.array(T), "meta/pad_token_id": np.array(PAD), "meta/kind": np.array(kind),
           "meta/dataset": np.array(str(dataset)), "meta/guided": np.array(guided),
           "meta/txt_cond": np.array([s[0] for s in call_specs]), "meta/do_unconditional": np.array([s[1] for s in call_specs])}
    for k, v in eval_kw.items():
        if k != "_kw" and v is not None:
            out[f"meta/eval/{k}"] = np.array(v)
    for k, v in batch.items():
        if torch.is_tensor(v):
            out[f"batch/{k}"] = MG._np(v)
    unweighed_final = bool(eval_kw.get("return_unweighed_sim", False)) or (kind == "likelihood" and eval_kw.get("_kw", {}).get("return_unweighed", True))
    floors = []
    for c, (txt_cond, do_unc) in enumerate(call_specs):
        x0 = tr.qxt[c * T]["x0"]
        call = dict(x0=x0)
        steps = []
        for i in range(T):
            q, t = tr.qxt[c * T + i], tr.ts[c * T + i]
            f = tr.fwd[(c * T + i) * per:(c * T + i + 1) * per]
            assert torch.equal(q["x0"], x0)
            st = dict(t=t, u=q["u"], xt=q["xt"], inp_cond=f[0]["inp"], logits_cond=f[0]["logits"])
            if guided:
                st.update(inp_uncond=f[1]["inp"], logits_uncond=f[1]["logits"],
                          w=refeval.cfg(d.config, t, torch.stack([torch.zeros(t.shape[0], 1, 1), -torch.ones(t.shape[0], 1, 1)])).reshape(-1).expand(t.shape[0]).clone())
            steps.append(st)
        weighted, unweighed = tr.stacks[2 * c], tr.stacks[2 * c + 1]
        final = (unweighed if unweighed_final else weighted).mean(dim=0)
        if kind == "likelihood":
            assert torch.equal(final, ret["final"])
            cond_mask, valid = None, batch["attention_mask"]
        else:
            cond_mask = torch.zeros_like(x0, dtype=torch.bool)
            if txt_cond:
                cond_mask[:, :Lt] = True
            else:
                cond_mask[:, Lt:] = True
            valid = x0 != PAD
        out[f"call{c}/x0"], out[f"call{c}/weighted"], out[f"call{c}/unweighed"], out[f"call{c}/final"] = MG._np(x0), MG._np(weighted), MG._np(unweighed), MG._np(final)
        if detail_calls is not None and c not in detail_calls:
            continue
        for i, st in enumerate(steps):
            for k, v in st.items():
                out[f"call{c}/step{i}/{k}"] = MG._np(v)
        # the restated statements on the oracle's fp32 forward must reproduce the reference's scores; the bf16-emulating forward gives the noise floor
        w32, u32 = oracle_scores(case_name, params, call, steps, guided, do_unc, cond_mask, valid, modality, bf16=False)
        assert rel_err(w32, weighted) < 2e-5 and rel_err(u32, unweighed) < 2e-5, (name, c, rel_err(w32, weighted), rel_err(u32, unweighed))
        w16, u16 = oracle_scores(case_name, params, call, steps, guided, do_unc, cond_mask, valid, modality, bf16=True)
        out[f"call{c}/emu_weighted"], out[f"call{c}/emu_unweighed"] = MG._np(w16), MG._np(u16)
        out[f"floor/call{c}/weighted"], out[f"floor/call{c}/unweighed"] = np.array(rel_err(w16, weighted)), np.array(rel_err(u16, unweighed))
        floors.append((rel_err(w16, weighted), rel_err(u16, unweighed)))
    finals = [torch.from_numpy(out[f"call{c}/final"]) for c in range(n_calls)]
    if kind == "zero_shot":
        for m in METRICS:
            v = getattr(d, m).values
            if v:
                out[f"metric/{m}"] = np.array(v)
        if dataset == "facebook/winoground":
            # calls: modes image, text, group, each s0_0, s0_1, s1_0, s1_1 (model_eval.py:516-554); lower is better (:506-514)
            flags = {}
            for mi, mode in enumerate(("image", "text", "group")):
                s00, s01, s10, s11 = finals[4 * mi:4 * mi + 4]
                text_ok = torch.logical_and(s00 < s10, s11 < s01)
                image_ok = torch.logical_and(s00 < s01, s11 < s10)
                flags[mode] = dict(text=text_ok, image=image_ok)
            text_f, image_f = flags["text"]["text"], flags["image"]["image"]
            group_f = torch.logical_and(text_f, image_f) if eval_kw.get("wino_group_conditional", False) else torch.logical_and(flags["group"]["image"], flags["group"]["text"])
            B = text_f.shape[0]
            assert abs(float(text_f.sum()) / B - out["metric/win_text_accuracy"][0]) < 1e-12 and abs(float(image_f.sum()) / B - out["metric/win_image_accuracy"][0]) < 1e-12
            assert abs(float(group_f.sum()) / B - out["metric/win_group_accuracy"][0]) < 1e-12
            out["flags/text_correct"], out["flags/image_correct"], out["flags/group_correct"] = MG._np(text_f), MG._np(image_f), MG._np(group_f)
        elif eval_kw.get("only_one_correct", False):
            out["flags/argmin"] = np.array(int(finals[0].argmin()))
            assert float(int(finals[0].argmin()) == 0) == out["metric/datacomp_img_acc"][0]
        else:
            out["flags/txt_argmin"], out["flags/img_argmin"] = np.array(int(finals[0].argmin())), np.array(int(finals[1].argmin()))
            assert float(int(finals[1].argmin()) == 0) == out["metric/datacomp_img_acc"][0] and float(int(finals[0].argmin()) == 0) == out["metric/datacomp_txt_acc"][0]
    path = os.path.join(MG.GOLDEN_DIR, f"similarity_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f"{name}: calls={n_calls} floors(weighted, unweighed)={[(f'{a:.2e}', f'{b:.2e}') for a, b in floors]} "
          f"finals={[np.round(out[f'call{c}/final'], 4).tolist() for c in range(n_calls)]} -> {path} ({size / 1024:.0f} KiB)")
    return tr.signature, d


def main():
    RET = [(True, False), (False, False)]          # retrieval: get_similarity(x0_txt, txt_cond=True), get_similarity(x0_img, txt_cond=False)
    ONE = [(True, True)]                           # only_one_correct: get_similarity(x0c, do_unconditional=True)
    MODES = ("image", "text", "group")             # Winoground: per mode s0_0, s0_1, s1_0, s1_1 (model_eval.py:516-535)
    WINO = [(m != "text", m == "group") for m in MODES for _ in range(4)]
    sig, _ = record("b_small_retrieval", "b_small", dict(cfg=None), "datacomp", "zero_shot", RET)
    record("b_small_one_correct_unweighed", "b_small", dict(cfg=None, only_one_correct=True, return_unweighed_sim=True), "datacomp", "zero_shot", ONE)
    record("b_small_retrieval_cfg", "b_small", dict(cfg=1.5), "datacomp", "zero_shot", RET)
    record("b_small_one_correct_cfg_forced", "b_small", dict(cfg=1.5, force_cfg_value=True, only_one_correct=True), "datacomp", "zero_shot", ONE)
    # the Winoground-style branch is ONE run of 12 calls; its per-timestep records exceed the size limit of a committed file, so the same run (same seed) is
    # written once per mode with that mode's four calls in detail - every file holds all twelve calls' scores, the metric updates and the flags
    for mi, mode in enumerate(MODES):
        record(f"b_small_wino_{mode}", "b_small", dict(cfg=None), "facebook/winoground", "zero_shot", WINO, detail_calls=set(range(4 * mi, 4 * mi + 4)))
    record("b_small_wino_group_conditional", "b_small", dict(cfg=None, wino_group_conditional=True), "facebook/winoground", "zero_shot", WINO, detail_calls=set())
    record("b_small_likelihood", "b_small", dict(cfg=None, _kw=dict(return_unweighed=True)), None, "likelihood", [(True, True)])
    record("b_small_likelihood_weighted", "b_small", dict(cfg=None, _kw=dict(return_unweighed=False)), None, "likelihood", [(True, True)], detail_calls=set())
    record("c_large_retrieval", "c_large", dict(cfg=None), "datacomp", "zero_shot", RET)
    record("c_large_likelihood", "c_large", dict(cfg=None, _kw=dict(return_unweighed=True)), None, "likelihood", [(True, True)])
    import model_eval as refeval   # (module-level functions there; model.py:87-94 attaches them to Diffusion)

    sigs = {"reference": "alexanderswerdlow/unidisc (checkout under /root/reference)",
            "Diffusion": {"get_similarity": [dict(name="self", kind="POSITIONAL_OR_KEYWORD", default=None, has_default=False)] + sig,
                          "get_model_likelihood_score": describe(refeval.get_model_likelihood_score),
                          "zero_shot_eval_step": describe(refeval.zero_shot_eval_step)},
            "note": "get_similarity is nested in zero_shot_eval_step in the reference (model_eval.py:268); as a method here it gains `self`"}
    p = os.path.join(MG.GOLDEN_DIR, "signatures_similarity.json")
    with open(p, "w") as f:
        json.dump(sigs, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", p)


if __name__ == "__main__":
    main()
