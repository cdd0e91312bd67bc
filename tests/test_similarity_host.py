"""Host logic of zero-shot likelihood scoring (`Diffusion.get_similarity`, `get_model_likelihood_score`, `zero_shot_eval_step`) on the CPU with kernel
doubles (tests/fake_kernels_similarity.py), against the runs recorded from the imported reference by scripts/make_golden_similarity.py
(model_eval.py:263-652, :3569-3609; CPU fp32, eval mode, T = 4).

Pinned per recorded run: t, x_t and the model inputs of every timestep bit for bit (the recorded uniforms go in through `_rand`), the rows given to the
head = the contributing set, the guidance weights, the retrieval / Winoground flags on the recorded scores, the three signatures, the refusals, and that
stacking k timesteps per backbone pass changes nothing in x_t.

Not pinned as a run of the reference: nothing here - every branch listed in the fixtures ran in the reference itself.  One accommodation was needed to run
it at all: the checked-out `get_similarity` unpacks five of `q_xt`'s six return values (model_eval.py:319 / model.py:584); the generator's wrapper around
`q_xt` hands back the first five ("Zero-shot likelihood scoring").  The Winoground run is one run of twelve calls stored as three files."""
import inspect
import json
import os

import pytest
import torch

import fake_kernels_similarity as FK
from golden_utils import GOLDEN_DIR
from similarity_utils import Sim, loglinear, replay_rand, valid_ids

ZERO_SHOT = ["b_small_retrieval", "b_small_one_correct_unweighed", "b_small_retrieval_cfg", "b_small_one_correct_cfg_forced", "c_large_retrieval"]
LIKELIHOOD = ["b_small_likelihood", "c_large_likelihood"]
WINO = ["b_small_wino_image", "b_small_wino_text", "b_small_wino_group"]


@pytest.fixture
def doubles(monkeypatch):
    from unidisc_amd import diffusion as diff_mod, dit as dit_mod

    monkeypatch.setattr(dit_mod, "K", FK)
    monkeypatch.setattr(diff_mod, "K", FK)


class RecordedHead:
    """Stands in for `backbone.forward_masked_logits`: checks nothing itself, serves the REFERENCE's recorded logits (rounded to bf16) of the rows that
    `plan_ids` marks, in the product's order ([MASK] rows of plan_ids first, ascending), and keeps every call for the assertions."""

    def __init__(self, diff, logits_by_input):
        self.diff, self.logits_by_input, self.calls = diff, logits_by_input, []

    def __call__(self, xt, sigma=None, modality=None, sample_ids=None, plan_ids=None, block_mask=None):
        assert sigma is None and sample_ids is None and block_mask is None
        R, L = xt.shape
        V = self.diff.vocab_size
        Vp = (V + 127) // 128 * 128
        full = torch.full((R * L, Vp), float("nan"), dtype=torch.bfloat16)       # (columns past V: the kernels must not read them into a result)
        for r in range(0, R, self.B):
            full[r * L:(r + self.B) * L, :V] = self.logits_by_input(xt[r:r + self.B]).reshape(self.B * L, V).bfloat16()
        is_mask = (plan_ids.reshape(-1) == self.diff.mask_index)
        order = torch.argsort((~is_mask).to(torch.int8), stable=True)
        n = int(is_mask.sum())
        n_pad = min((max(n, 1) + 63) // 64 * 64, R * L)
        rows = order[:n_pad]
        self.calls.append(dict(xt=xt.clone(), plan_ids=plan_ids.clone(), modality=modality, rows=rows[:n].clone()))
        return full.index_select(0, rows), rows, n


def _logits_lookup(sim, calls):
    """model input [B, L] -> the reference's fp32 logits for it (both halves of a guided pass are inputs of their own)"""
    table = []
    for c in calls:
        for i in range(sim.T):
            table.append((sim.t(f"call{c}/step{i}/inp_cond"), sim.t(f"call{c}/step{i}/logits_cond")))
            if sim.guided:
                table.append((sim.t(f"call{c}/step{i}/inp_uncond"), sim.t(f"call{c}/step{i}/logits_uncond")))

    def lookup(x):
        for inp, lg in table:
            if torch.equal(inp, x):
                return lg
        raise AssertionError("the product ran the backbone on an input the reference never saw")

    return lookup


def _fp64_scores(sim, diff, c, valid, cond_mask, do_unc):
    """The reference's statements (model_eval.py:331-370) in fp64 on ITS logits rounded to bf16 -> weighted, unweighed [T, B] and the per-sample bound that
    the per-row kernel tolerance atol = 2e-4 (1 + 2 w) (tests/test_gpu_similarity_kernels.py) plus fp32 summation allows."""
    x0 = sim.t(f"call{c}/x0")
    B, L = x0.shape
    V, Vt, mask = diff.vocab_size, diff.text_vocab_size, diff.mask_index
    modality = sim.t("batch/modality")
    ok = valid_ids(V, Vt, mask, modality.reshape(-1), diff._restrict()).reshape(B, L, V)
    ws, us, bw, bu = [], [], [], []
    for i in range(sim.T):
        t, xt = sim.t(f"call{c}/step{i}/t"), sim.t(f"call{c}/step{i}/xt")
        z = sim.t(f"call{c}/step{i}/logits_cond").bfloat16().double()
        wmax = 0.0
        if sim.guided:
            w = sim.t(f"call{c}/step{i}/w").double().reshape(B, 1, 1)
            z = (1 + w) * z - w * sim.t(f"call{c}/step{i}/logits_uncond").bfloat16().double()
            wmax = float(w.max())
        z = z.masked_fill(~ok, float("-inf"))
        log_p = z.gather(-1, x0[..., None]).squeeze(-1) - torch.logsumexp(z, -1)
        contributes = (xt == mask) & valid
        if cond_mask is not None and not do_unc:
            contributes = contributes & ~cond_mask
        log_p = torch.where(contributes, log_p, torch.zeros_like(log_p))
        sigma, dsigma = loglinear(t.double())
        w_std = (dsigma / torch.expm1(sigma))
        cnt = valid.sum(-1).double()
        ws.append((-log_p * w_std[:, None]).sum(-1) / cnt)
        us.append((-log_p).sum(-1) / cnt)
        tok = (2e-4 * (1 + 2 * wmax) + 1e-5 * log_p.abs()) * contributes          # per-row tolerance of the log-probability
        n = contributes.sum(-1).double()
        slack = (n + 2) * 2.0 ** -24                                              # fp32 summation of n terms and the division
        bu.append((tok.sum(-1) + slack * log_p.abs().sum(-1)) / cnt)
        bw.append((tok.sum(-1) + slack * log_p.abs().sum(-1)) * w_std * (1 + 2.0 ** -22) / cnt)   # (w_std itself is an fp32 value: a few ulp)
    return torch.stack(ws), torch.stack(us), torch.stack(bw), torch.stack(bu)


def _check_trace(sim, diff, trace, head_calls, calls, k=1):
    """t, x_t, inputs bit for bit; the rows of the head = the contributing set; the guidance weights"""
    assert len(trace) == len(calls) * sim.T
    Lt = diff.config.model.txt_length
    for ci, c in enumerate(calls):
        x0 = sim.t(f"call{c}/x0")
        B, L = x0.shape
        valid = sim.t("batch/attention_mask").bool() if sim.kind == "likelihood" else x0 != sim.pad
        for i in range(sim.T):
            tr, key = trace[ci * sim.T + i], f"call{c}/step{i}"
            assert torch.equal(tr["t"], sim.t(f"{key}/t")), key
            assert torch.equal(tr["xt"], sim.t(f"{key}/xt")), key
            assert torch.equal(tr["cond"], sim.t(f"{key}/inp_cond")), key
            want = (tr["xt"] == diff.mask_index) & valid
            if sim.kind != "likelihood" and not sim.do_unconditional[c]:
                cond_mask = torch.zeros_like(x0, dtype=torch.bool)
                if sim.txt_cond[c]:
                    cond_mask[:, :Lt] = True
                else:
                    cond_mask[:, Lt:] = True
                want = want & ~cond_mask
            assert torch.equal(tr["contributes"], want), key
            if sim.guided:
                assert torch.equal(tr["uncond"], sim.t(f"{key}/inp_uncond")), key
                assert torch.equal(tr["w"], sim.t(f"{key}/w")), key                 # the reference's own `cfg` weight, bit for bit
    # the head ran on exactly the contributing rows (every pass: k timesteps of one call, stacked)
    per_call = (sim.T + k - 1) // k
    passes = [h for h in head_calls]
    if sim.guided and getattr(diff.config.eval, "split_cfg_batches", False):
        assert all(torch.equal(a["rows"], b["rows"]) for a, b in zip(passes[0::2], passes[1::2]))
        passes = passes[0::2]
    assert len(passes) == len(calls) * per_call
    for ci in range(len(calls)):
        for p in range(per_call):
            steps = range(p * k, min((p + 1) * k, sim.T))
            want = torch.cat([trace[ci * sim.T + i]["contributes"] for i in steps], 0).reshape(-1).nonzero().reshape(-1)
            rows = passes[ci * per_call + p]["rows"]
            if sim.guided and not getattr(diff.config.eval, "split_cfg_batches", False):
                n = rows.numel() // 2
                assert torch.equal(rows[n:], rows[:n] + len(steps) * trace[0]["xt"].numel())     # the same positions of the unconditional half
                rows = rows[:n]
            assert torch.equal(rows, want)


def _run(sim, diff):
    if sim.kind == "likelihood":
        return diff.get_model_likelihood_score(sim.batch(), num_timesteps=sim.T)
    return diff.zero_shot_eval_step(sim.batch(), 0)


@pytest.mark.parametrize("name,split", [(n, False) for n in ZERO_SHOT + LIKELIHOOD] + [(n, True) for n in ZERO_SHOT if "cfg" in n])
def test_scores_replay_reference_run_on_its_logits(name, split, doubles, monkeypatch):
    """The whole host path on the reference's OWN logits (served, rounded to bf16, by a stand-in for the backbone): per timestep t / x_t / inputs / rows /
    weights as recorded, and the per-timestep scores within the kernel tolerance of the fp64 restatement on the same bf16 logits."""
    sim = Sim(name)
    assert sim.guided or not split
    diff = sim.product("cpu", split_cfg_batches=split)
    calls = sim.detailed_calls()
    assert calls == list(range(sim.n_calls))
    queue = replay_rand(diff, monkeypatch, sim.uniforms())
    head = RecordedHead(diff, _logits_lookup(sim, calls))
    head.B = sim.t("call0/x0").shape[0]
    monkeypatch.setattr(diff.backbone, "forward_masked_logits", head)
    got_w, got_u = [], []
    orig = diff._likelihood_scores

    def spy(*a, **k):
        w, u = orig(*a, **k)
        got_w.append(w), got_u.append(u)
        return w, u

    monkeypatch.setattr(diff, "_likelihood_scores", spy)
    diff._similarity_trace = trace = []
    out = _run(sim, diff)
    assert not queue, "the product made fewer draws than the reference"
    _check_trace(sim, diff, trace, head.calls, calls)
    Lt = diff.config.model.txt_length
    for c in calls:
        x0 = sim.t(f"call{c}/x0")
        cond_mask = None
        valid = sim.t("batch/attention_mask").bool()
        if sim.kind != "likelihood":
            cond_mask = torch.zeros_like(x0, dtype=torch.bool)
            cond_mask[:, :Lt] = True
            cond_mask = cond_mask if sim.txt_cond[c] else ~cond_mask
            valid = x0 != sim.pad
        w64, u64, bw, bu = _fp64_scores(sim, diff, c, valid, cond_mask, sim.do_unconditional[c])
        assert ((got_w[c].double() - w64).abs() <= bw).all(), (name, c, (got_w[c].double() - w64).abs().max(), bw.min())
        assert ((got_u[c].double() - u64).abs() <= bu).all(), (name, c, (got_u[c].double() - u64).abs().max(), bu.min())
    if sim.kind == "likelihood":
        assert torch.equal(out, got_u[0].mean(0))


@pytest.mark.parametrize("name", ["b_small_retrieval", "b_small_retrieval_cfg", "b_small_likelihood", "c_large_retrieval"])
def test_host_path_through_the_backbone_doubles(name, doubles, monkeypatch):
    """The same replay through the real `DIT.forward_masked_logits` on the CPU doubles (plan_ids, sigma = None, the [cond ; uncond] batch): the trace and
    the row selection are the recorded ones and every score is finite."""
    sim = Sim(name)
    diff = sim.product("cpu")
    calls = sim.detailed_calls()
    queue = replay_rand(diff, monkeypatch, sim.uniforms())
    head_calls = []
    orig = diff.backbone.forward_masked_logits

    def fml(xt, sigma=None, **k):
        logits, rows, n = orig(xt, sigma, **k)
        head_calls.append(dict(rows=rows[:n].clone()))
        return logits, rows, n

    monkeypatch.setattr(diff.backbone, "forward_masked_logits", fml)
    diff._similarity_trace = trace = []
    out = _run(sim, diff)
    assert not queue
    _check_trace(sim, diff, trace, head_calls, calls)
    scores = [out] if sim.kind == "likelihood" else [out["txt_class_sim"], out["img_class_sim"]]
    for s in scores:
        assert s.shape == (sim.t("call0/x0").shape[0],) and torch.isfinite(s).all()


@pytest.mark.parametrize("name", ["b_small_retrieval", "b_small_retrieval_cfg", "b_small_likelihood"])
@pytest.mark.parametrize("k", [2, 3])
def test_stacked_timesteps_draw_and_corrupt_like_one_per_pass(name, k, doubles, monkeypatch):
    """eval.similarity_timesteps_per_pass = k: the draws are still made per timestep in ascending order, x_t / inputs / weights are bit-identical to k = 1
    (= the recorded ones), every pass's head rows are the k timesteps' contributing rows, and - on the served reference logits, where the backbone cannot
    differ - the scores are bit-identical too."""
    sim = Sim(name)
    calls = sim.detailed_calls()
    outs = {}
    for kk in (1, k):
        diff = sim.product("cpu", similarity_timesteps_per_pass=kk)
        queue = replay_rand(diff, monkeypatch, sim.uniforms())
        head = RecordedHead(diff, _logits_lookup(sim, calls))
        head.B = sim.t("call0/x0").shape[0]
        monkeypatch.setattr(diff.backbone, "forward_masked_logits", head)
        diff._similarity_trace = trace = []
        out = _run(sim, diff)
        assert not queue
        _check_trace(sim, diff, trace, head.calls, calls, k=kk)
        assert max(h["xt"].shape[0] for h in head.calls) == kk * head.B * (2 if sim.guided else 1)
        outs[kk] = out if sim.kind == "likelihood" else torch.stack([out["txt_class_sim"], out["img_class_sim"]])
    assert torch.equal(outs[1], outs[k])


def _serve_recorded_scores(sim, diff, monkeypatch):
    """get_similarity returns the reference's final scores call by call; the arguments of every call are checked against the recorded ones"""
    state = dict(c=0)

    def get_similarity(x0, batch, num_timesteps=None, txt_cond=True, return_unweighed=False, do_unconditional=False):
        c = state["c"]
        assert torch.equal(x0, sim.t(f"call{c}/x0")), c
        assert do_unconditional == sim.do_unconditional[c], c
        if not do_unconditional:
            assert txt_cond == sim.txt_cond[c], c
        state["c"] += 1
        return sim.t(f"call{c}/final")

    monkeypatch.setattr(diff, "get_similarity", get_similarity)
    return state


@pytest.mark.parametrize("name", ZERO_SHOT)
def test_retrieval_flags_on_recorded_scores(name, monkeypatch):
    """DataComp-style branches (model_eval.py:567-652): the candidate tensors handed to get_similarity are the reference's (the rolled image halves of
    eval.only_one_correct; text or image fixed to row 0 otherwise) and, on its scores, the accuracies are the ones it reported."""
    sim = Sim(name)
    diff = sim.product("cpu")
    state = _serve_recorded_scores(sim, diff, monkeypatch)
    out = diff.zero_shot_eval_step(sim.batch(), 0)
    assert state["c"] == sim.n_calls
    assert out["datacomp_img_acc"] == float(sim.t("metric/datacomp_img_acc")[0])
    assert diff.zero_shot_metric("datacomp_img_acc") == float(sim.t("metric/datacomp_img_acc")[0])
    if sim.eval_kw.get("only_one_correct", False):
        assert int(out["class_sim"].argmin()) == int(sim.t("flags/argmin"))
    else:
        assert out["datacomp_txt_acc"] == float(sim.t("metric/datacomp_txt_acc")[0])
        assert int(out["txt_class_sim"].argmin()) == int(sim.t("flags/txt_argmin")) and int(out["img_class_sim"].argmin()) == int(sim.t("flags/img_argmin"))


@pytest.mark.parametrize("name", ["b_small_wino_image", "b_small_wino_group_conditional"])
def test_winoground_flags_on_recorded_scores(name, monkeypatch):
    """Winoground-style branch (model_eval.py:479-566): twelve calls in the reference's order (modes image, text, group; pairs 0_0, 0_1, 1_0, 1_1) with
    its txt_cond / do_unconditional, and text / image / group correctness per row as recorded - with and without eval.wino_group_conditional."""
    sim = Sim(name)
    diff = sim.product("cpu")
    state = _serve_recorded_scores(sim, diff, monkeypatch)
    out = diff.zero_shot_eval_step(sim.batch(), 0)
    assert state["c"] == 12
    for mode in ("text", "image", "group"):
        assert torch.equal(out[f"{mode}_correct"], sim.t(f"flags/{mode}_correct").bool()), mode
        assert out[f"win_{mode}_accuracy"] == float(sim.t(f"metric/win_{mode}_accuracy")[0])
    assert diff.zero_shot_metric("win_group_accuracy") == out["win_group_accuracy"]


@pytest.mark.parametrize("name", WINO)
def test_winoground_modes_replay_reference_run(name, doubles, monkeypatch):
    """The Winoground run is one run of twelve calls stored as three files, each with one mode's four calls in detail: those four replay (t, x_t, inputs,
    rows) through get_similarity with the mode's txt_cond / do_unconditional, on the reference's logits, within the kernel tolerance of fp64."""
    sim = Sim(name)
    diff = sim.product("cpu")
    calls = sim.detailed_calls()
    assert len(calls) == 4
    replay_rand(diff, monkeypatch, sim.uniforms(calls))
    head = RecordedHead(diff, _logits_lookup(sim, calls))
    head.B = sim.t("call0/x0").shape[0]
    monkeypatch.setattr(diff.backbone, "forward_masked_logits", head)
    diff._similarity_trace = trace = []
    Lt = diff.config.model.txt_length
    finals = [diff.get_similarity(sim.t(f"call{c}/x0"), sim.batch(), txt_cond=sim.txt_cond[c], do_unconditional=sim.do_unconditional[c]) for c in calls]
    _check_trace(sim, diff, trace, head.calls, calls)
    for c, f in zip(calls, finals):
        x0 = sim.t(f"call{c}/x0")
        cond_mask = torch.zeros_like(x0, dtype=torch.bool)
        cond_mask[:, :Lt] = True
        cond_mask = cond_mask if sim.txt_cond[c] else ~cond_mask
        w64, _, bw, _ = _fp64_scores(sim, diff, c, x0 != sim.pad, cond_mask, sim.do_unconditional[c])
        assert ((f.double() - w64.mean(0)).abs() <= bw.mean(0) + 2.0 ** -22 * w64.mean(0).abs()).all(), c


def test_signatures_match_the_reference():
    """names, kinds and defaults of the three methods as recorded from the reference (get_similarity is nested there and gains `self` here); the product may
    append keyword parameters with defaults, never reorder."""
    import unidisc_amd

    sig = json.load(open(os.path.join(GOLDEN_DIR, "signatures_similarity.json")))["Diffusion"]
    assert sorted(sig) == ["get_model_likelihood_score", "get_similarity", "zero_shot_eval_step"]
    for method, ref in sig.items():
        got = [dict(name=p.name, kind=p.kind.name, has_default=p.default is not inspect.Parameter.empty,
                    default=None if p.default is inspect.Parameter.empty else repr(p.default))
               for p in inspect.signature(getattr(unidisc_amd.Diffusion, method)).parameters.values()]
        assert got[:len(ref)] == ref, method
        assert all(p["has_default"] for p in got[len(ref):]), method


def test_random_timesteps_are_sorted_draws(doubles, monkeypatch):
    """eval.use_random_timesteps_same_batch / _diff_batch (model_eval.py:279-287): rand(T), or rand(B, T), sorted ascending, drawn BEFORE the first q_xt
    draw; per-sample times reach the schedule per sample."""
    sim = Sim("b_small_retrieval")
    B, L = sim.t("call0/x0").shape
    g = torch.Generator().manual_seed(5)
    for flag, shape in (("use_random_timesteps_same_batch", (sim.T,)), ("use_random_timesteps_diff_batch", (B, sim.T))):
        diff = sim.product("cpu", **{flag: True})
        times = torch.rand(*shape, generator=g)
        replay_rand(diff, monkeypatch, [times] + sim.uniforms([0]))
        diff._similarity_trace = trace = []
        diff.get_similarity(sim.t("call0/x0"), sim.batch(), num_timesteps=sim.T)
        want = torch.sort(times)[0]
        for i, tr in enumerate(trace):
            assert torch.equal(tr["t"], want[:, i] if want.dim() == 2 else want[i].expand(B))
            u = sim.t(f"call0/step{i}/u")
            move = 1 - torch.exp(-loglinear(tr["t"])[0][:, None])
            assert torch.equal(tr["xt"] == diff.mask_index, (u < move) | (sim.t("call0/x0") == diff.mask_index))


def test_cfg_weight_forms():
    """`cfg` (model_eval.py:2630-2640): eval.cfg (1 - t); linspace(0, 10, B) (1 - t) for -1; the scalar under force_cfg_value; no timestep windows."""
    sim = Sim("b_small_retrieval_cfg")
    t = torch.tensor([0.2, 0.4, 0.6, 0.8])
    diff = sim.product("cpu", cfg=1.5, cfg_min_timestep=0.5, cfg_max_timestep=0.7)
    assert torch.equal(diff._similarity_cfg_weight(t), 1.5 * (1 - t))
    diff = sim.product("cpu", cfg=-1)
    assert torch.equal(diff._similarity_cfg_weight(t), torch.linspace(0, 10, 4) * (1 - t))
    diff = sim.product("cpu", cfg=2.5, force_cfg_value=True)
    assert torch.equal(diff._similarity_cfg_weight(t), torch.full((4,), 2.5))


def test_sample_without_valid_tokens_scores_nan(doubles, monkeypatch):
    """a row of nothing but padding: 0 / 0 = NaN, as in the reference (model_eval.py:369); the other rows are untouched by it"""
    sim = Sim("b_small_retrieval")
    diff = sim.product("cpu")
    x0 = sim.t("call0/x0").clone()
    x0[2] = sim.pad
    replay_rand(diff, monkeypatch, sim.uniforms([0]))
    s = diff.get_similarity(x0, sim.batch(), num_timesteps=sim.T)
    assert torch.isnan(s[2]) and torch.isfinite(s[[0, 1, 3]]).all()


def test_refusals(doubles):
    """every option that is not built raises NotImplementedError naming it"""
    sim = Sim("b_small_retrieval")
    x0, batch = sim.t("call0/x0"), sim.batch()

    def refuses(match, fn):
        with pytest.raises(NotImplementedError, match=match):
            fn()

    diff = sim.product("cpu", wino_chameleon=True)
    refuses("wino_chameleon", lambda: diff.zero_shot_eval_step(batch, 0))
    diff = sim.product("cpu")
    diff.config.data.train = "nlphuji/flickr30k"
    refuses("flickr30k", lambda: diff.zero_shot_eval_step(batch, 0))
    diff = sim.product("cpu")
    diff.config.model.img_first = True
    refuses("img_first", lambda: diff.zero_shot_eval_step(batch, 0))
    refuses("img_first", lambda: diff.get_similarity(x0, batch, num_timesteps=2))
    refuses("img_first", lambda: diff.get_model_likelihood_score(batch, num_timesteps=2))
    diff = sim.product("cpu")
    diff.time_conditioning = True
    refuses("time_conditioning", lambda: diff.get_similarity(x0, batch, num_timesteps=2))
    refuses("time_conditioning", lambda: diff.get_model_likelihood_score(batch, num_timesteps=2))
    refuses("time_conditioning", lambda: diff.zero_shot_eval_step(batch, 0))
    diff = sim.product("cpu")
    packed = dict(batch, sample_ids=torch.zeros_like(batch["modality"]))
    refuses("sample_ids", lambda: diff.get_similarity(x0, packed, num_timesteps=2))
    refuses("sample_ids", lambda: diff.get_model_likelihood_score(packed, num_timesteps=2))
    refuses("sample_ids", lambda: diff.zero_shot_eval_step(packed, 0))
    diff = sim.product("cpu")
    diff.config.eval.pad_token_id = None
    with pytest.raises(ValueError, match="pad"):
        diff.get_similarity(x0, batch, num_timesteps=2)


def test_kernel_doubles_agree_with_the_existing_cross_entropy_double():
    """fake subs_logp_rows without guidance = fake subs_ce_fwd's log_p on all-masked rows (the property the HIP kernels hold bit for bit)"""
    g = torch.Generator().manual_seed(0)
    M, V, Vt, mask = 12, 65, 41, 40
    logits = torch.randn(M, 72, generator=g).bfloat16()
    mod = (torch.arange(M) % 2).long()
    x0 = torch.where(mod == 1, torch.randint(Vt, V, (M,), generator=g), torch.randint(0, Vt - 1, (M,), generator=g))
    lp, _ = FK.subs_ce_fwd(logits, x0, torch.full((M,), mask), mod, V, Vt, mask, True)
    assert torch.equal(FK.subs_logp_rows(logits, x0, mod, V, Vt, mask, True), lp)
    w, u = FK.likelihood_scores(lp, torch.arange(M), torch.tensor([2.0, 3.0, 1.0]), torch.tensor([4.0, 8.0, 0.0]), 6)
    assert torch.allclose(u[:2], torch.stack([-lp[:6].sum() / 4, -lp[6:].sum() / 8])) and torch.allclose(w[:2], u[:2] * torch.tensor([2.0, 3.0]))
    assert torch.isnan(u[2]) and torch.isnan(w[2])


def test_ar_similarity_on_forward(monkeypatch):
    """parameterization=ar (model_eval.py:380-422): `get_similarity_ar` = the reference's statements on `Diffusion.forward`'s next-token log-probs - the
    whole-row NLL is the count-weighted mean of its text and image parts - and `zero_shot_eval_step` routes retrieval to it."""
    from ar_utils import ArGolden, build_ar_product
    from test_ar import _fake_with_causal
    from unidisc_amd import diffusion as diff_mod, dit as dit_mod

    fk = _fake_with_causal()                       # (the kernel doubles with the causal attention double of tests/test_ar.py)
    monkeypatch.setattr(dit_mod, "K", fk)
    monkeypatch.setattr(diff_mod, "K", fk)
    g = ArGolden("ar_b_small")
    diff = build_ar_product(g, "cpu")
    diff.backbone.eval()
    pad = 7
    diff.config.eval.pad_token_id = pad
    diff.config.data.train = "datacomp"
    batch = diff.update_batch(g.batch())
    x0 = torch.where(batch["attention_mask"], batch["input_ids"], torch.full_like(batch["input_ids"], pad))
    Lt = diff.config.model.txt_length
    nll = diff.get_similarity_ar(x0, batch, do_unconditional=True)
    img, txt = diff.get_similarity_ar(x0, batch, txt_cond=True), diff.get_similarity_ar(x0, batch, txt_cond=False)
    with torch.no_grad():
        lp = diff.forward(x=x0, sigma=None, modality=batch["modality"]).float().gather(-1, x0[:, 1:, None])[..., 0]
    am = x0[:, 1:] != pad
    assert torch.allclose(nll, (-lp * am).sum(-1) / am.sum(-1))
    n_t, n_i = am[:, :Lt - 1].sum(-1), am[:, Lt - 1:].sum(-1)
    assert torch.allclose(nll * (n_t + n_i), txt * n_t + img * n_i, rtol=1e-5)
    out = diff.zero_shot_eval_step(dict(batch, input_ids=x0), 0)
    assert out["txt_class_sim"].shape == (x0.shape[0],) and torch.isfinite(out["img_class_sim"]).all()
    with pytest.raises(NotImplementedError, match="img_first"):
        diff.get_similarity_ar(x0, batch, img_first=True)
    with pytest.raises(ValueError, match="get_similarity_ar"):
        diff.get_similarity(x0, batch, num_timesteps=2)
