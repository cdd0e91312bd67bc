"""What the host sampler asks of the kernels, case by case: `Diffusion.sample()` and `get_similarity` over a matrix of configurations on the `c_large` and
`b_small` products, with every call the sampler makes recorded in order - each `K.*` call of unidisc_amd/diffusion.py and each
`backbone.forward_masked_logits` call, as (name, digest of every tensor argument, scalars) - plus the returned tokens, `nfe` and `sample_step_modes`.  A
combination the product refuses is recorded as its exception type and text.  Two runs of this script on two versions of diffusion.py that print the same
file made the same calls with the same operands and returned the same tokens: the check a refactor of the host sampler is held to.

    python scripts/trace_sampler.py --out new.json                               # CPU, kernel doubles (tests/fake_kernels_reveal.py + the two scoring doubles)
    python scripts/trace_sampler.py --out old.json --diffusion /path/to/another/diffusion.py   # the same on another version of the file
    python scripts/trace_sampler.py --compare old.json new.json                  # cases, traced calls, how many differ
    python scripts/trace_sampler.py --device cuda --matrix small --out gpu.json  # the real kernels, a short matrix (AR sampler included)

`--diffusion` loads the given file as a module of the package (relative imports work), so both versions run on the same dit.py and kernels."""
import argparse
import hashlib
import importlib.util
import inspect
import itertools
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

PREDICTORS = ("ddpm_cache", "maskgit", "maskgit_nucleus", "first_hitting")
EOS, PAD, BOS = 2, 0, 1
STEPS = 4


class Tok:
    eos_token_id, pad_token_id, bos_token_id = EOS, PAD, BOS


VOCAB = [None]   # the product's vocabulary size: logits are [rows, Vp] with the columns past V padding that no kernel reads (and nothing initialises)


def digest(v):
    if isinstance(v, torch.Tensor):
        if v.dim() == 2 and v.is_floating_point() and VOCAB[0] is not None and v.shape[1] > VOCAB[0]:
            v = v[:, :VOCAB[0]]
        t = v.detach().cpu().contiguous()
        raw = t.view(torch.uint8).numpy().tobytes() if t.numel() else b""
        return f"T:{str(t.dtype)[6:]}{list(t.shape)}:{hashlib.sha1(raw).hexdigest()[:12]}"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, dict):
        return {str(k): digest(x) for k, x in sorted(v.items())}
    if isinstance(v, torch.Generator):
        return "Generator"
    if hasattr(v, "__dict__"):   # ModalityMask and the like: the class and its tensors
        return {type(v).__name__: digest({k: x for k, x in vars(v).items() if not k.startswith("_")})}
    return type(v).__name__


class TracedK:
    """the kernel module the sampler sees: every function call is appended to `trace` before it runs"""

    def __init__(self, real, trace):
        self.__dict__["_real"], self.__dict__["_trace"] = real, trace

    def __getattr__(self, name):
        obj = getattr(self._real, name)
        if not isinstance(obj, (types.FunctionType, types.BuiltinFunctionType)):
            return obj

        def call(*a, **kw):
            if name.endswith("_supported"):   # host predicates on dtype / device / the row length: no launch, and the rows they are shown do not matter
                self._trace.append([f"K.{name}", [f"{str(v.dtype)[6:]}{list(v.shape[1:])}" if isinstance(v, torch.Tensor) else digest(v) for v in a]])
            else:
                self._trace.append([f"K.{name}", digest(a), digest(kw)])
            return obj(*a, **kw)

        return call


def load_modules(path, device):
    """(diffusion module, dit module, kernel namespace): the package's own diffusion.py, or the file at `path` loaded as another module of the package"""
    from unidisc_amd import diffusion as diff_mod, dit as dit_mod
    if path is not None:
        spec = importlib.util.spec_from_file_location("unidisc_amd._diffusion_under_trace", path)
        diff_mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = diff_mod
        spec.loader.exec_module(diff_mod)
    if device == "cpu":
        import fake_kernels_reveal as FK
        import fake_kernels_similarity as FS
        kern = types.SimpleNamespace(**{k: v for k, v in vars(FK).items() if not k.startswith("__")})
        kern.subs_logp_rows, kern.likelihood_scores = FS.subs_logp_rows, FS.likelihood_scores
        dit_mod.K = kern
    else:
        from unidisc_amd import kernels as kern
    return diff_mod, dit_mod, kern


class Runner:
    def __init__(self, path, device):
        self.device = device
        self.diff_mod, self.dit_mod, self.kern = load_modules(path, device)
        self.trace = []
        self.diff_mod.K = TracedK(self.kern, self.trace)
        self.results = {}

    def product(self, case, ar=False, multimodal=True, **ev):
        from golden_utils import Golden
        from product_utils import product_config
        from unidisc_amd.config import Cfg
        if ar:
            from ar_utils import ArGolden, ar_config
            g = ArGolden(f"ar_{case}")
            cfg = ar_config(g.case)
        else:
            g = Golden(case)
            cfg = product_config(g.case if multimodal else dict(g.case, multimodal_batches=False))   # (False: no `modality` argument, the static slices)
        diff = self.diff_mod.Diffusion(cfg, None, self.device)
        diff.backbone.load_state_dict(g.params(), strict=True)
        diff.backbone.to(self.device)
        diff.backbone.eval()
        diff.config.eval = Cfg(maskgit_r_temp=10.0, **ev)
        VOCAB[0] = diff.vocab_size
        real, trace = diff.backbone.forward_masked_logits, self.trace

        defaults = {k: p.default for k, p in inspect.signature(real).parameters.items()}

        def traced_forward(*a, **kw):   # (a keyword passed at its default value and one left out are the same call: neither is recorded)
            said = {k: v for k, v in kw.items() if not (k in defaults and (v is defaults[k] or (isinstance(v, int) and v == defaults[k])))}
            trace.append(["forward_masked_logits", digest(a), digest(said)])
            return real(*a, **kw)

        diff.backbone.forward_masked_logits = traced_forward
        return diff, g

    def run(self, cid, fn):
        """fn() -> dict of results; the trace of the calls it made and what it raised go with it"""
        assert cid not in self.results, cid
        del self.trace[:]
        torch.manual_seed(1234)
        try:
            out = fn()
        except Exception as e:  # noqa: BLE001 - a refusal is a result
            if "HIP error" in str(e) or "illegal memory access" in str(e):   # (a device fault is not: nothing more runs on that GPU)
                raise
            out = dict(error=[type(e).__name__, str(e)])
        self.results[cid] = dict(out, calls=len(self.trace), trace=[list(c) for c in self.trace])


def conditioning(g, diff, B, kind, seed=0):
    """x0 / x0_unmask for "none" | "partial" | "text" | "image" (that modality fully given), and the modality map"""
    Lt, Li = g.case["txt_length"], g.case["img_length"]
    Vt, V = g.case["text_vocab_size"], g.case["vocab_size"]
    gen = torch.Generator().manual_seed(1000 + seed)
    x0 = torch.cat([torch.randint(3, diff.mask_index, (B, Lt), generator=gen), torch.randint(Vt, V, (B, Li), generator=gen)], 1)
    x0[:, Lt // 2] = EOS     # (an EOS inside the text, for the padding rule)
    unmask = torch.zeros(B, Lt + Li, dtype=torch.bool)
    if kind == "partial":
        unmask = torch.rand(B, Lt + Li, generator=gen) < 0.4
    elif kind == "text":
        unmask[:, :Lt] = True
    elif kind == "image":
        unmask[:, Lt:] = True
    modality = torch.cat([torch.zeros(B, Lt, dtype=torch.int64), torch.ones(B, Li, dtype=torch.int64)], 1)
    return (None, None, modality) if kind == "none" else (x0, unmask, modality)


GUIDANCE = {"none": {}, "cfg": dict(cfg=1.5), "split": dict(cfg=1.5, split_cfg_batches=True),
            "window": dict(cfg=1.5, cfg_min_timestep=0.4, cfg_max_timestep=0.8),        # t = 1, .75, .5, .25: no weight at the first and the last step
            "window_split": dict(cfg=1.5, cfg_min_timestep=0.4, cfg_max_timestep=0.8, split_cfg_batches=True),
            "forced": dict(cfg=2.0, force_cfg_value=True)}


def sample_case(r, cid, case, predictor, guidance, cond, *, cc=False, mod=True, pad=False, fused=False, fused_nucleus=False, nr=True, seed=3, steps=STEPS, B=None, **ev):
    if B is None:   # (get_cfg_weight's timestep window broadcasts [B] against [B, 1]: with x0 it runs at B = 1 only; one B = 2 case records the error)
        B = 1 if guidance.startswith("window") else 2

    def fn():
        kw = dict(GUIDANCE[guidance], fused_reveal=fused, fused_nucleus=fused_nucleus, top_p=0.95, temperature=0.9, **ev)
        if cc:
            kw["conditioning_cache"] = True
        diff, g = r.product(case, multimodal=mod, **kw)
        diff.tokenizer = Tok()
        diff.config.trainer.force_after_eos_padding = pad
        x0, unmask, modality = conditioning(g, diff, B, cond)
        dev = r.device
        args = dict(num_steps=steps, predictor=predictor, seed=seed, noise_removal=nr, return_nfe=True)
        if x0 is not None:
            args.update(x0=x0.to(dev), x0_unmask=unmask.to(dev))
        else:
            args.update(batch_size=B)
        if mod:
            args.update(modality=modality.to(dev))
        x, nfe = diff.sample(**args)
        return dict(tokens=x.cpu().tolist(), nfe=int(nfe), modes=list(diff.sample_step_modes))
    r.run(cid, fn)


def similarity_case(r, cid, case, guidance, k, txt_cond, do_unc, likelihood=False):
    def fn():
        diff, g = r.product(case, pad_token_id=PAD, similarity_timesteps_per_pass=k, **GUIDANCE[guidance])
        from unidisc_amd.config import Cfg
        diff.config.sampling = Cfg(steps=STEPS)
        B = 3
        x0, _, modality = conditioning(g, diff, B, "text", seed=5)
        x0[:, g.case["txt_length"] - 3:g.case["txt_length"]] = PAD
        dev = r.device
        x0, modality = x0.to(dev), modality.to(dev)
        batch = dict(input_ids=x0, modality=modality, attention_mask=x0 != PAD)
        diff._similarity_trace = rec = []
        if likelihood:
            s = diff.get_model_likelihood_score(batch, num_timesteps=STEPS)
        else:
            s = diff.get_similarity(x0, batch, txt_cond=txt_cond, do_unconditional=do_unc)
        return dict(scores=digest(s), values=[float(v) for v in s.cpu()], steps=digest([sorted(d.items()) for d in rec]))
    r.run(cid, fn)


def ar_cases(r):
    def refuse(cid, what):
        def fn():
            diff, g = r.product("b_small", ar=True)
            what(diff)
            return dict(ok=True)
        r.run(cid, fn)

    L = 32
    x0, um = torch.zeros(2, L, dtype=torch.int64), torch.zeros(2, L, dtype=torch.bool)

    def as_cuda(diff):
        diff.device = torch.device("cuda")     # past the device check: the argument checks come before any GPU work
    if r.device == "cpu":
        refuse("ar/cpu/_ar_sampler", lambda d: d._ar_sampler(2))
        refuse("ar/cpu/sample", lambda d: d.sample(batch_size=2))
        refuse("ar/cpu/sample_sample_ids", lambda d: d.sample(batch_size=2, sample_ids=x0))
        refuse("ar/cpu/cfg", lambda d: (setattr(d.config.eval, "cfg", 1.5), d.sample(batch_size=2, x0=x0, x0_unmask=um)))
        for key, kw in (("sample_ids", dict(sample_ids=x0)), ("replay", dict(replay=[None])), ("predictor", dict(predictor="maskgit")), ("num_steps", dict(num_steps=5))):
            refuse(f"ar/args/{key}", lambda d, kw=kw: (as_cuda(d), d.sample(batch_size=2, **kw)))
        refuse("ar/cfg_without_force", lambda d: (as_cuda(d), setattr(d.config.eval, "cfg", 1.5), d._ar_sampler(2, x0=x0, x0_unmask=um, bos_token_id=1)))
        refuse("ar/cfg_window", lambda d: (as_cuda(d), setattr(d.config.eval, "cfg", 1.5), setattr(d.config.eval, "force_cfg_value", True),
                                           setattr(d.config.eval, "cfg_min_timestep", 0.2), d._ar_sampler(2, x0=x0, x0_unmask=um, bos_token_id=1)))
        refuse("ar/no_bos", lambda d: (as_cuda(d), d._ar_sampler(2)))
        refuse("ar/conditioning_cache", lambda d: (setattr(d.config.eval, "conditioning_cache", True), d.sample(batch_size=2)))
        return
    for case in ("b_small", "c_large"):
        for name, ev, given in (("plain", {}, False), ("x0", {}, True), ("guided", dict(cfg=2.0, force_cfg_value=True), True), ("top_p", dict(top_p=0.9, temperature=0.8), True),
                                ("top_p_guided", dict(top_p=0.9, temperature=0.8, cfg=2.0, force_cfg_value=True), True),
                                ("top_p_fused", dict(top_p=0.9, temperature=0.8, fused_nucleus=True), False)):
            def fn(case=case, ev=ev, given=given):
                diff, g = r.product(case, ar=True, **ev)
                B = 2
                c0, cu, modality = conditioning(g, diff, B, "text")
                cu[:, 0] = False
                kw = dict(x0=c0.to(r.device), x0_unmask=cu.to(r.device)) if given else {}
                diff.tokenizer = Tok()
                x, nfe = diff.sample(batch_size=B, modality=modality.to(r.device), seed=7, return_nfe=True, **kw)
                return dict(tokens=x.cpu().tolist(), nfe=int(nfe))
            r.run(f"ar/{case}/{name}", fn)


def helper_cases(r):
    """the sampler's pieces that tests and scripts call by name, on seeded inputs"""
    def fn():
        diff, g = r.product("c_large", cfg=1.5, cfg_min_timestep=0.4, cfg_max_timestep=0.8)
        dev = r.device
        gen = torch.Generator().manual_seed(5)
        V = diff.vocab_size
        z = (torch.randn(300, V + 7, generator=gen) * 3).to(dev)
        zu = (torch.randn(300, V + 7, generator=gen) * 3).to(dev)
        w = torch.rand(300, generator=gen).to(dev)
        rm = (torch.arange(300) % 2).to(dev)
        out = dict(nucleus=digest(diff._nucleus_draw(z, None, None, None, 0.9, 0.8, 11)), nucleus_guided=digest(diff._nucleus_draw(z, zu, w, rm, 0.9, 0.8, 11)))
        zz = z[:, :V].float().masked_fill((torch.arange(V, device=dev) == diff.mask_index)[None], float("-inf"))
        out["ar_nucleus"] = digest(diff._ar_nucleus(zz, 0.9, 0.8, torch.Generator(device=dev).manual_seed(3)))
        x = torch.randint(0, V, (3, 32), generator=gen).to(dev)
        x[:, 5] = EOS
        mod = (torch.arange(32) >= 16).long().expand(3, 32).to(dev)
        out["pad"] = digest(diff._pad_after_eos(x, (EOS, PAD), mod))
        rows = torch.tensor([0, 17, 40, 95], device=dev)
        out["row_modality"] = [digest(diff._row_modality(rows, 3, 32, None)), digest(diff._row_modality(rows, 3, 32, mod))]
        out["sche"] = [digest(diff.adap_sche(torch.where(x < 30, diff.mask_index, x), 4, diff.mask_index, m)) for m in ("arccos", "linear")]
        out["cfg_w"] = [digest(diff.get_cfg_weight(torch.full((3,), t, device=dev))) for t in (1.0, 0.75, 0.5, 0.25)]
        out["eos_ids"] = [repr(diff._eos_padding_ids(False)), repr(diff._eos_padding_ids(True))]
        return out
    r.run("helpers", fn)


def full_matrix(r):
    preds = [(p, False) for p in PREDICTORS] + [("maskgit_nucleus", True)]
    # A: the structure - predictor x guidance x conditioning x conditioning cache x modality given or the static slices
    for (p, fn_), gd, cond, cc, mod in itertools.product(preds, GUIDANCE, ("none", "partial", "text", "image"), (False, True), (True, False)):
        case = "c_large" if mod else "b_small"   # (c_large's 2-D rope needs the modality argument)
        sample_case(r, f"A/{case}/{p}{'+fn' if fn_ else ''}/{gd}/{cond}/cc{int(cc)}/mod{int(mod)}", case, p, gd, cond, cc=cc, mod=mod, fused_nucleus=fn_)
    # B: the step tail - padding x fused reveal x noise removal
    for (p, fn_), gd, cond, cc, pad, fused, nr in itertools.product(preds, ("none", "cfg"), ("none", "partial", "text", "image"), (False, True), (False, True), (False, True),
                                                                    (True, False)):
        if not (pad or fused or not nr):
            continue   # (in A)
        sample_case(r, f"B/c_large/{p}{'+fn' if fn_ else ''}/{gd}/{cond}/cc{int(cc)}/pad{int(pad)}/fused{int(fused)}/nr{int(nr)}", "c_large", p, gd, cond, cc=cc, pad=pad,
                    fused=fused, fused_nucleus=fn_, nr=nr)
    # C: eval.attention_caching - ratio x read cache x number of steps (a run ends sliced or unsliced) x modality x padding key x noise removal
    for ratio, rc, steps, mod, pad, nr in itertools.product((2, 3), (False, True), (4, 5, 6, 7), (True, False), (False, True), (True, False)):
        case = "c_large" if mod else "b_small"
        sample_case(r, f"C/{case}/ratio{ratio}/read{int(rc)}/steps{steps}/mod{int(mod)}/pad{int(pad)}/nr{int(nr)}", case, "ddpm_cache", "none", "none", mod=mod, pad=pad,
                    nr=nr, steps=steps, attention_caching=True, attention_caching_txt_to_img_ratio=ratio, attention_caching_read_cache=rc)
    for name, p, gd, cond, ev in (("maskgit", "maskgit", "none", "none", {}), ("x0", "ddpm_cache", "none", "partial", {}), ("cfg", "ddpm_cache", "cfg", "none", {}),
                                  ("cc", "ddpm_cache", "none", "text", dict(conditioning_cache=True)), ("fused", "ddpm_cache", "none", "none", dict(fused=True, pad=True))):
        sample_case(r, f"C/refused_or_not/{name}", "c_large", p, gd, cond, attention_caching=True, attention_caching_txt_to_img_ratio=2, **ev)
    # D: the second product, seeds from the global generator, an unknown predictor, B = 1
    for p, gd, cond, cc in itertools.product(PREDICTORS, ("none", "cfg", "split", "window"), ("none", "text", "image"), (False, True)):
        sample_case(r, f"D/b_small/{p}/{gd}/{cond}/cc{int(cc)}", "b_small", p, gd, cond, cc=cc)
    for p in PREDICTORS:
        sample_case(r, f"D/c_large/{p}/global_seed", "c_large", p, "cfg", "partial", seed=None, pad=True)
        sample_case(r, f"D/c_large/{p}/B1", "c_large", p, "split", "text", B=1, cc=True, pad=True, fused=True)
    sample_case(r, "D/c_large/window_B2", "c_large", "maskgit", "window", "text", B=2)
    sample_case(r, "D/c_large/unknown_predictor", "c_large", "euler", "none", "none")
    # E: the likelihood score
    for case, gd, k, txt_cond, do_unc in itertools.product(("c_large", "b_small"), ("none", "cfg", "split", "forced"), (1, 2), (True, False), (False, True)):
        similarity_case(r, f"E/{case}/{gd}/k{k}/txt{int(txt_cond)}/unc{int(do_unc)}", case, gd, k, txt_cond, do_unc)
    for case, k in itertools.product(("c_large", "b_small"), (1, 2, 3)):
        similarity_case(r, f"E/{case}/likelihood/k{k}", case, "none", k, True, True, likelihood=True)
    ar_cases(r)
    helper_cases(r)


def small_matrix(r):
    """the short matrix for the real kernels: seeded, 4 steps"""
    for case in ("c_large", "b_small"):
        for p, gd, (cond, cc) in itertools.product(PREDICTORS, ("none", "cfg", "split"), (("none", False), ("partial", False), ("text", True), ("image", True))):
            sample_case(r, f"S/{case}/{p}/{gd}/{cond}/cc{int(cc)}", case, p, gd, cond, cc=cc)
        for p in PREDICTORS:
            sample_case(r, f"S/{case}/{p}/tail", case, p, "cfg", "text", pad=True, fused=True, fused_nucleus=True)
            sample_case(r, f"S/{case}/{p}/pad", case, p, "window", "partial", pad=True, nr=False)
        for ratio, rc, steps in itertools.product((2, 3), (False, True), (4, 5)):
            sample_case(r, f"S/{case}/caching/ratio{ratio}/read{int(rc)}/steps{steps}", case, "ddpm_cache", "none", "none", steps=steps, attention_caching=True,
                        attention_caching_txt_to_img_ratio=ratio, attention_caching_read_cache=rc)
        for gd, k in itertools.product(("none", "cfg", "split"), (1, 2)):
            similarity_case(r, f"S/{case}/similarity/{gd}/k{k}", case, gd, k, True, False)
    ar_cases(r)
    helper_cases(r)


def compare(a, b, outcome_only=False):
    with open(a) as f:
        ra = json.load(f)
    with open(b) as f:
        rb = json.load(f)
    strip = (lambda c: {k: v for k, v in c.items() if k not in ("trace", "calls")}) if outcome_only else (lambda c: c)
    ids = sorted(set(ra) | set(rb))
    differ = [i for i in ids if i not in ra or i not in rb or strip(ra[i]) != strip(rb[i])]
    refused = sum(1 for i in ids if "error" in ra.get(i, {}))
    print(json.dumps(dict(cases=len(ids), refused=refused, traced_calls=[sum(c["calls"] for c in ra.values()), sum(c["calls"] for c in rb.values())],
                          compared="outcomes" if outcome_only else "traces and outcomes", differ=len(differ), first_differing=differ[:10])))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--diffusion", default=None, help="another version of unidisc_amd/diffusion.py to run instead of the package's")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--matrix", default="full", choices=("full", "small"))
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--outcome-only", action="store_true", help="--compare: tokens, nfe, step modes and errors only (not the traces)")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, outcome_only=a.outcome_only))
    r = Runner(a.diffusion, a.device)
    {"full": full_matrix, "small": small_matrix}[a.matrix](r)
    refused = sum(1 for c in r.results.values() if "error" in c)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r.results, f, sort_keys=True)
    print(json.dumps(dict(cases=len(r.results), refused=refused, traced_calls=sum(c["calls"] for c in r.results.values()))))


if __name__ == "__main__":
    main()
