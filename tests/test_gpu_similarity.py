"""Zero-shot likelihood scoring end to end on a real MI355X (pytest -m gpu): `Diffusion.zero_shot_eval_step` / `get_model_likelihood_score` on the draws the
imported reference made (tests/golden/similarity_*.npz, scripts/make_golden_similarity.py; `b_small`, T = 4) against the reference's fp32 scores.

THE BOUND is measured, not chosen: the fixture holds, per recorded call, the same per-timestep scores computed from the oracle's bf16-emulating forward
(oracle/unidisc_oracle.py `dit_forward(bf16=True)` - the path of test_bf16_emulation_within_reference_noise_floor) on the recorded model inputs; its
relative distance ||s_emu - s_ref|| / ||s_ref|| over the [T, B] scores of a call is the noise floor of running this model in bf16 at all, and the product
must stay within 2x that floor (the project's per-parameter margin).  Achieved value and bound go to the parity ledger.

Arg-min agreement on the model's scores is NOT asserted: the candidates of an untrained model are near-ties (the flags are pinned on the recorded scores in
tests/test_similarity_host.py).

Every branch in the fixtures ran in the reference itself; the one accommodation (its `get_similarity` unpacks five of `q_xt`'s six values, so the
generator's wrapper hands back five) is described in DESIGN.md."""
import pytest
import torch

from golden_utils import rel_err
from ledger import check
from similarity_utils import Sim, replay_rand

pytestmark = pytest.mark.gpu
DEV = "cuda"
RUNS = ["b_small_retrieval", "b_small_one_correct_unweighed", "b_small_retrieval_cfg", "b_small_one_correct_cfg_forced", "b_small_likelihood", "c_large_retrieval"]


def _spy(diff, monkeypatch):
    got = []
    orig = diff._likelihood_scores

    def spy(*a, **k):
        w, u = orig(*a, **k)
        got.append((w.float().cpu(), u.float().cpu()))
        return w, u

    monkeypatch.setattr(diff, "_likelihood_scores", spy)
    return got


def _run(sim, diff):
    if sim.kind == "likelihood":
        return diff.get_model_likelihood_score(sim.batch(DEV), num_timesteps=sim.T)
    return diff.zero_shot_eval_step(sim.batch(DEV), 0)


def _product_scores(sim, monkeypatch, **eval_extra):
    diff = sim.product(DEV, **eval_extra)
    queue = replay_rand(diff, monkeypatch, sim.uniforms())
    got = _spy(diff, monkeypatch)
    diff._similarity_trace = trace = []
    out = _run(sim, diff)
    torch.cuda.synchronize()
    assert not queue and len(got) == sim.n_calls
    for c in range(sim.n_calls):                       # the corruption is the reference's, bit for bit
        for i in range(sim.T):
            assert torch.equal(trace[c * sim.T + i]["xt"].cpu(), sim.t(f"call{c}/step{i}/xt")), (c, i)
    return diff, got, out, trace


@pytest.mark.parametrize("name", RUNS)
def test_scores_within_twice_the_bf16_floor_of_the_reference(name, monkeypatch):
    """per recorded call: ||s - s_ref|| / ||s_ref|| over the [T, B] per-timestep scores, weighted and unweighed, <= 2 x the recorded bf16-emulation floor"""
    sim = Sim(name)
    _, got, out, _ = _product_scores(sim, monkeypatch)
    test = f"test_scores_within_twice_the_bf16_floor_of_the_reference[{name}]"
    for c in range(sim.n_calls):
        for j, form in enumerate(("weighted", "unweighed")):
            floor = float(sim.t(f"floor/call{c}/{form}"))
            ach = rel_err(got[c][j], sim.t(f"call{c}/{form}"))
            print(f"{name} call{c} {form}: achieved {ach:.3e}, floor {floor:.3e}, bound {2 * floor:.3e}")
            check(test, f"call{c}/{form}_rel_err_vs_reference_fp32 (floor {floor:.3e})", ach, 2.0 * floor)
    finals = [out] if sim.kind == "likelihood" else ([out["class_sim"]] if "class_sim" in out else [out["txt_class_sim"], out["img_class_sim"]])
    unweighed_final = sim.kind == "likelihood" or bool(sim.eval_kw.get("return_unweighed_sim", False))
    for c, f in enumerate(finals):                     # the returned score is the mean over the timesteps of the selected form
        assert torch.equal(f.cpu(), got[c][1 if unweighed_final else 0].mean(0))


@torch.no_grad()
def _unfused_scores(sim, diff, trace, c):
    """The unfused composition on the SAME x_t: full [B, L, V] logits from `Diffusion.forward`, then the reference's tensor statements
    (model_eval.py:320-370) in fp32 torch.  Unguided, the SUBS log-probs are `Diffusion.forward`'s own kernel (`_subs_parameterization`) asked for fp32
    output - its default bf16 output rounds every log-prob by up to 2^-9 relative, forty times the kernel bound this comparison is held to; guided, the
    reference's `_subs_parameterization` statements on the fp32 mixture (the product's kernel takes bf16 logits only)."""
    x0 = sim.t(f"call{c}/x0").to(DEV)
    B, L = x0.shape
    modality = sim.t("batch/modality").to(DEV)
    batch = dict(modality=modality)
    Lt = diff.config.model.txt_length
    V, Vt, mask = diff.vocab_size, diff.text_vocab_size, diff.mask_index
    if sim.kind == "likelihood":
        cond_mask, valid, do_unc = None, sim.t("batch/attention_mask").bool().to(DEV), True
    else:
        cond_mask = torch.zeros_like(x0, dtype=torch.bool)
        cond_mask[:, :Lt] = True
        cond_mask = cond_mask if sim.txt_cond[c] else ~cond_mask
        valid, do_unc = x0 != sim.pad, sim.do_unconditional[c]
    ws, us, bound, w_stds = [], [], [], []
    for i in range(sim.T):
        tr = trace[c * sim.T + i]
        xt, t = tr["xt"], tr["t"]
        lc = diff.forward(tr["cond"], None, batch=batch, modality=modality, return_logits=True)
        wmax = 0.0
        if sim.guided:
            lu = diff.forward(tr["uncond"], None, batch=batch, modality=modality, return_logits=True)
            w = tr["w"][:, None, None]
            z = (1 + w) * lc.float() - w * lu.float()
            ar = torch.arange(V, device=DEV)
            ok = torch.where((modality == 1)[..., None], ar >= Vt, ar < Vt) if diff._restrict() else torch.ones(B, L, V, dtype=torch.bool, device=DEV)
            ok = ok & (ar != mask)
            z = z.masked_fill(~ok, diff.neg_infinity)
            lp = z - torch.logsumexp(z, -1, keepdim=True)
            unmasked = (xt != mask)[..., None]
            lp = torch.where(unmasked, torch.where(ar == xt[..., None], 0.0, diff.neg_infinity), lp)
            wmax = float(tr["w"].max())
        else:
            lp = diff._subs_parameterization(lc.float(), xt=xt, batch=batch, modality=modality)
            assert lp.dtype == torch.float32
        log_p = torch.gather(lp.float(), -1, x0[:, :, None]).squeeze(-1)
        log_p = torch.where(valid, log_p, torch.zeros_like(log_p))
        if not do_unc:
            log_p = torch.where(cond_mask, torch.zeros_like(log_p), log_p)
        sigma, dsigma = diff.noise(t)
        w_std = dsigma / torch.expm1(sigma)
        w_stds.append(w_std)
        cnt = valid.sum(-1)
        ws.append((-log_p * w_std[:, None]).sum(-1) / cnt)
        us.append((-log_p).sum(-1) / cnt)
        # what two evaluations of the same log-probabilities may differ by: twice the per-row kernel tolerance (tests/test_gpu_similarity_kernels.py:
        # atol 2e-4 (1 + 2 max w), rtol 1e-5) on every contributing row, and the fp32 summation of both sides
        n = (log_p != 0).sum(-1)
        tok = 2 * ((2e-4 * (1 + 2 * wmax)) * n + 1e-5 * log_p.abs().sum(-1)) + 2 * (n + 2) * 2.0 ** -24 * log_p.abs().sum(-1)
        bound.append(tok / cnt)
    return torch.stack(ws).cpu(), torch.stack(us).cpu(), torch.stack(bound).cpu(), torch.stack(w_stds).cpu()


@pytest.mark.parametrize("name", ["b_small_retrieval", "b_small_retrieval_cfg", "b_small_likelihood"])
def test_fused_equals_unfused_composition(name, monkeypatch):
    """the fused score (head on the contributing rows, udm_subs_logp_rows, udm_likelihood_scores) = the unfused composition on the same x_t within the
    kernel bounds, per timestep and sample"""
    sim = Sim(name)
    diff, got, _, trace = _product_scores(sim, monkeypatch)
    for c in range(sim.n_calls):
        w_ref, u_ref, bound, w_std = _unfused_scores(sim, diff, trace, c)
        du, dw = (got[c][1] - u_ref).abs(), (got[c][0] - w_ref).abs()
        print(f"{name} call{c}: max |fused - unfused| unweighed {float(du.max()):.3e} (bound >= {float(bound.min()):.3e}), weighted {float(dw.max()):.3e}")
        assert (du <= bound).all(), (c, float(du.max()), float(bound.min()))
        assert (dw <= bound * w_std * (1 + 2.0 ** -20)).all(), (c, float(dw.max()))


@pytest.mark.parametrize("extra", [dict(split_cfg_batches=True), dict(similarity_timesteps_per_pass=2), dict(similarity_timesteps_per_pass=4)],
                         ids=["split_cfg_batches", "k2", "k4"])
def test_split_batches_and_stacked_timesteps_agree(extra, monkeypatch):
    """eval.split_cfg_batches (two passes of B rows instead of one of 2 B) and eval.similarity_timesteps_per_pass (k B rows per pass): the same x_t bit for
    bit (checked in _product_scores against the recording), and scores that agree with the default form within the end-to-end bound - 2 x the bf16
    floor - and are themselves within it of the reference: a pass of another row count may be dispatched to another GEMM tile, so the bf16 logits, and
    with them the scores, are equal only up to bf16 rounding."""
    sim = Sim("b_small_retrieval_cfg")
    _, base, _, _ = _product_scores(sim, monkeypatch)
    _, other, _, _ = _product_scores(sim, monkeypatch, **extra)
    test = f"test_split_batches_and_stacked_timesteps_agree[{'-'.join(extra)}]"
    for c in range(sim.n_calls):
        for j, form in enumerate(("weighted", "unweighed")):
            floor = float(sim.t(f"floor/call{c}/{form}"))
            check(test, f"call{c}/{form}_rel_err_vs_default_form", rel_err(other[c][j], base[c][j]), 2.0 * floor)
            check(test, f"call{c}/{form}_rel_err_vs_reference_fp32", rel_err(other[c][j], sim.t(f"call{c}/{form}")), 2.0 * floor)
