"""fp64 reference, acceptance rule and input families for the fused top-p kernels (csrc/nucleus.hip: udm_nucleus_sample_rows, udm_ar_nucleus_rows).

The rule (one routine for both reference samplers):
    valid ids      id < V, id != mask_id and, under `restrict`, the row's modality only
    z              logits, or (1 + w) logits - w logits_uncond, every operation rounded to fp32 (what torch does to fp32-promoted logits)
    p              softmax(inv_temperature z) over the valid ids
    order          descending p, ascending id among equal values (the stable order)
    kept           the longest prefix with S(n) = p_(1) + ... + p_(n) <= budget; n >= 1
    token          argmax over the kept ids of p_i / (1e-10 - log(fl32(u_i + 1e-10))), first index on ties
`nucleus_sampling_batch` (model_eval.py:2642-2685) is inv_temperature = 1, budget = top_p * temperature; `nucleus_sampling` (:2691-2734) is
inv_temperature = 1 / temperature, budget = top_p.

Here: z in fp32 exactly as above, everything after it in fp64.

Acceptance of a kept count n (every row, none excluded): n is the exact prefix length for SOME budget within delta of the requested one,
    (n == 1 or S(n) <= budget + delta)   and   (n == n_valid or S(n + 1) > budget - delta).

delta.  A kernel holds e_i = fl(exp2(a_i)), a_i = fl(fl(z_i - z_max) * scale), scale = fl(inv_temperature * log2(e)), and compares fixed-order fp32 sums:
mass(prefix) <= fl(budget * Z).
  * sums: a sum of n non-negative fp32 terms in any order is off by at most (n - 1) 2^-24 relative; prefix mass and Z each are, and the product
    budget * Z adds one rounding.  The project's column-sum form covers the three together: (n_valid + 8) 2^-24 budget.
  * the exponent argument: z_i - z_max rounds once (2^-24 relative), scale carries the rounding of log2(e) and of its product (2 * 2^-24), the product
    a_i one more: |a_i - a_i exact| <= THETA |a_i| with THETA = 4 * 2^-24, which moves e_i by the factor exp(ln 2 * a_i * THETA): relative
    A THETA, where A = inv_temperature * (z_max - z_min over the valid ids) bounds ln 2 |a_i|.  The hardware exp2 adds 1 ulp = 2^-23.  Numerator and Z
    move independently, hence the 2:   2 budget (A THETA + 2^-23).
    (a_i below -126 flushes e_i to 0: an absolute loss of at most n_valid 2^-126, below anything above.)
delta = (n_valid + 8) 2^-24 budget + 2 budget (4 * 2^-24 A + 2^-23).
"""
import math

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TOP_P, TEMPERATURE = 0.95, 0.9                      # the demo's setting
RULES = {"batch": (1.0, TOP_P * TEMPERATURE), "ar": (1.0 / TEMPERATURE, TOP_P)}     # name -> (inv_temperature, budget)
THETA = 4 * 2.0 ** -24
RACE_MARGIN = 2.0 ** -18                            # rows whose two best race values are closer than this (relative) are not held to the token
FAMILIES = ("gauss", "peak", "flat", "ramp", "plateaus", "neg300", "spikes")
LSE_ATOL, LSE_RTOL = 2e-4, 1e-5                     # the bound of udm_subs_logp_rows (tests/rowops_ref64.py)


def valid_ids(M, V, Vt, mask_id, modality, restrict, mutant=None):
    ar = torch.arange(V)[None]
    v = torch.ones(M, V, dtype=torch.bool)
    if restrict:
        v = torch.where((modality == 1)[:, None], ar >= Vt, ar < Vt).clone()
    if mutant != "forbidden_kept":
        v[:, mask_id] = False
    return v


def mix32(zc, zu, w, V):
    """fp32 [M, V]: the guided logits, each operation rounded (w fp32 [M] or None)"""
    z = zc[:, :V].to(F32)
    if zu is not None:
        wv = w.to(F32)[:, None]
        z = (1 + wv) * z - wv * zu[:, :V].to(F32)
    return z


def probs64(z32, valid, inv_t):
    a = (z32.double() * inv_t).masked_fill(~valid, float("-inf"))
    return torch.softmax(a, -1)


def stable_order(p, valid, descending_ids=False):
    """ids [M, V] in kept order: descending p, ascending id among equals; invalid ids last"""
    key = torch.where(valid, -p, torch.full_like(p, float("inf")))
    if descending_ids:
        o = torch.sort(key.flip(-1), dim=-1, stable=True)[1]
        return p.shape[1] - 1 - o
    return torch.sort(key, dim=-1, stable=True)[1]


def delta_of(z32, valid, inv_t, budget):
    zz = z32.double()
    span = zz.masked_fill(~valid, float("-inf")).amax(-1) - zz.masked_fill(~valid, float("inf")).amin(-1)
    n_valid = valid.sum(-1).double()
    return (n_valid + 8) * 2.0 ** -24 * budget + 2 * budget * (THETA * inv_t * span + 2.0 ** -23)


class Ref:
    """everything the checks need, computed once per (inputs, rule)"""

    def __init__(self, zc, zu, w, valid, inv_t, budget, V):
        self.V, self.valid, self.inv_t, self.budget = V, valid, inv_t, budget
        self.z32 = mix32(zc, zu, w, V)
        self.p = probs64(self.z32, valid, inv_t)
        self.order = stable_order(self.p, valid)
        self.S = self.p.gather(1, self.order).cumsum(-1)          # S[:, n - 1] = S(n)
        self.n_valid = valid.sum(-1)
        self.delta = delta_of(self.z32, valid, inv_t, budget)
        self.n = torch.clamp(((self.S <= budget) & (torch.arange(V)[None] < self.n_valid[:, None])).sum(-1), min=1)      # the exact count
        self.logp1 = torch.log_softmax(self.z32.double().masked_fill(~valid, float("-inf")), -1)

    def accepts(self, keep):
        """bool [M]: the acceptance rule above"""
        keep = keep.long()
        ok = (keep >= 1) & (keep <= self.n_valid)
        k = keep.clamp(1, self.V)
        s_n = self.S.gather(1, (k - 1)[:, None])[:, 0]
        s_next = self.S.gather(1, k.clamp(max=self.V - 1)[:, None])[:, 0]
        first = (k == 1) | (s_n <= self.budget + self.delta)
        second = (k >= self.n_valid) | (s_next > self.budget - self.delta)
        return ok & first & second

    def race(self, keep, u):
        """(token [M], decided [M]): the fp64 race over the first keep[r] ids of the order; decided is False where the two best values are within RACE_MARGIN"""
        M, V = self.p.shape
        rank = torch.empty_like(self.order)
        rank.scatter_(1, self.order, torch.arange(V)[None].expand(M, V))
        inside = (rank < keep.long()[:, None]) & self.valid
        den = 1e-10 - torch.log((u[:, :V].to(F32) + 1e-10).double())
        score = torch.where(inside, self.p / den, torch.full_like(self.p, -1.0))
        top2 = torch.topk(score, min(2, V), dim=-1)
        tok = torch.where(score == top2.values[:, :1], torch.arange(V)[None].expand(M, V), torch.full((M, V), V)).amin(-1)      # first index on exact ties
        if V > 1:
            second = top2.values[:, 1].clamp(min=0.0)
            decided = (top2.values[:, 0] - second) > RACE_MARGIN * top2.values[:, 0]
        else:
            decided = torch.ones(M, dtype=torch.bool)
        return tok, decided

    def judge(self, keep, tok, u):
        """list of violations (empty = accepted): every row's count by the acceptance rule, every decided row's token by the race over that row's own prefix"""
        bad = []
        acc = self.accepts(keep)
        if not bool(acc.all()):
            r = int((~acc).nonzero()[0])
            bad.append(f"{int((~acc).sum())} rows with a kept count outside the rule, first row {r}: kept {int(keep[r])}, exact {int(self.n[r])}")
            keep = torch.where(acc, keep.long(), self.n)
        want, decided = self.race(keep, u)
        wrong = decided & (want != tok.long())
        if bool(wrong.any()):
            r = int(wrong.nonzero()[0])
            bad.append(f"{int(wrong.sum())} rows with another token than the race over their prefix, first row {r}: {int(tok[r])} vs {int(want[r])}")
        if int((~decided).sum()) * 100 > keep.shape[0]:
            bad.append(f"{int((~decided).sum())} of {keep.shape[0]} rows undecided (more than 1 %)")
        return bad


# ------------------------------------------------------------------------------------------------ fp32 emulations and mutants
def emulate(zc, zu, w, valid, inv_t, budget, u, V, arith="fp64", mutant=None):
    """(keep [M], token [M]) of an implementation of the rule.  arith: "fp64" | "seq32" (fp32 softmax, torch's sequential cumsum in sorted order, as the
    tensor path) | "hist32" (fp32 exp values, masses summed per distinct value from the top: the order of a histogram / radix selection).
    mutant: None or one of MUTANTS (fp64 arithmetic with one rule broken)."""
    M = zc.shape[0]
    z32 = mix32(zc, zu, w, V)
    dt = F64 if arith == "fp64" else F32
    a = (z32.to(dt) * torch.tensor(inv_t, dtype=dt)).masked_fill(~valid, float("-inf"))
    p = torch.softmax(a, -1)
    order = stable_order(p.double(), valid, descending_ids=(mutant == "ties_descending"))
    sp = p.gather(1, order)
    n_valid = valid.sum(-1)
    live = torch.arange(V)[None] < n_valid[:, None]
    if arith == "hist32":
        keep = torch.empty(M, dtype=torch.long)
        for r in range(M):
            e = torch.exp2(((z32[r] - z32[r][valid[r]].max()) * torch.tensor(inv_t * 1.4426950408889634, dtype=F32)))[valid[r]]
            vals, counts = torch.unique(e, return_counts=True)
            Z = torch.zeros((), dtype=F32)
            for v, c in zip(vals.flip(0), counts.flip(0)):
                Z = Z + v * c.to(F32)
            Bu = torch.tensor(budget, dtype=F32) * Z
            acc, n = torch.zeros((), dtype=F32), 0
            for v, c in zip(vals.flip(0), counts.flip(0)):
                m = acc + v * c.to(F32)
                if bool(m <= Bu):
                    acc, n = m, n + int(c)
                    continue
                if float(v) > 0:
                    n += max(0, min(int(c), int(torch.floor((Bu - acc) / v))))
                break
            keep[r] = max(n, 1)
    else:
        cum = sp.cumsum(-1)
        keep = ((cum <= torch.tensor(budget, dtype=dt)) & live).sum(-1)
        if mutant != "top_not_forced":
            keep = keep.clamp(min=1)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(V)[None].expand(M, V))
    inside = (rank < keep[:, None]) & valid
    den = 1e-10 - torch.log((u[:, :V].to(F32) + 1e-10).double())
    weight = p.double()
    if mutant == "uniform_draw":
        weight = torch.ones_like(weight)
    if mutant == "unfiltered_draw":
        inside = valid
    tok = torch.where(inside, weight / den, torch.full_like(weight, -1.0)).argmax(-1)
    return keep, tok


MUTANTS = ("top_not_forced", "budget_top_p", "temperature_on_logits", "ties_descending", "forbidden_kept", "uniform_draw", "unfiltered_draw")


def run_mutant(name, c, rule="batch"):
    """(keep, tok) of the mutant on case c under the batch rule (the only one `budget_top_p` and `temperature_on_logits` exist in)"""
    inv_t, budget = RULES[rule]
    valid = c["valid"]
    if name == "budget_top_p":
        budget = TOP_P
    if name == "temperature_on_logits":
        inv_t = 1.0 / TEMPERATURE
    if name == "forbidden_kept":
        valid = valid_ids(c["M"], c["V"], c["Vt"], c["mask_id"], c["modality"], c["restrict"], mutant=name)
    return emulate(c["zc"], c["zu"], c["w"], valid, inv_t, budget, c["u"], c["V"], mutant=name)


# ------------------------------------------------------------------------------------------------ inputs
def case(family, V, Vt, mask_id, M, *, restrict, guided, seed=0, ld=None):
    """dict: zc (and zu, w) bf16 [M, ld] finite everywhere, modality, valid, u fp32 [M, ld].  Rows alternate text / image when the vocabulary has an image
    part.  The caller poisons what the kernel must not read (poison())."""
    g = torch.Generator().manual_seed(7700 + 131 * FAMILIES.index(family) + V + 7 * M + 1000003 * seed)
    ld = ld or (V + 8 + 7) // 8 * 8                       # always padded past V
    two = V > Vt
    modality = (torch.arange(M) % 2).long() if two else torch.zeros(M, dtype=torch.long)
    valid = valid_ids(M, V, Vt, mask_id, modality, restrict and two)
    base = torch.randn(M, V, generator=g) * 2.0
    z = torch.zeros(M, ld)
    vcount = valid.sum(-1)
    if family == "gauss":
        z[:, :V] = base
    elif family == "peak":                                 # rows 0 mod 3: one peak; 1 mod 3: a tied peak of two; 2 mod 3: a tied peak of three, p = 1/3 each
        z[:, :V] = base
        for r in range(M):
            ids = valid[r].nonzero()[:, 0]
            pick = ids[torch.randperm(len(ids), generator=g)[:1 + r % 3]]
            z[r, pick] = 40.0
    elif family == "flat":
        z[:, :V] = 1.25
    elif family == "ramp":                                 # geometric: the j-th id of a random permutation of the valid ids at -j / 4 (bf16 rounds the far tail into ties)
        z[:, :V] = -60.0
        for r in range(M):
            ids = valid[r].nonzero()[:, 0]
            perm = ids[torch.randperm(len(ids), generator=g)]
            z[r, perm] = torch.clamp(-0.25 * torch.arange(len(ids)), min=-60.0)
    elif family == "plateaus":                             # n1 ids at 2, n2 ids at 0 scattered over the row, the rest at -30: the cut falls inside the second plateau
        z[:, :V] = -30.0
        for r in range(M):
            ids = valid[r].nonzero()[:, 0]
            n1 = max(1, len(ids) // 40)
            n2 = min(len(ids) - n1, 13 * n1 + r % 5)
            perm = ids[torch.randperm(len(ids), generator=g)]
            z[r, perm[:n1]] = 2.0
            z[r, perm[n1:n1 + n2]] = 0.0
    elif family == "neg300":
        z[:, :V] = base - 300.0
        for r in range(M):
            ids = valid[r].nonzero()[:, 0]
            z[r, ids[int(torch.randint(len(ids), (1,), generator=g))]] = 0.0
    elif family == "spikes":                               # +80 on every forbidden id
        z[:, :V] = base + torch.where(valid, 0.0, 80.0)
    else:
        raise ValueError(family)
    c = {"family": family, "V": V, "Vt": Vt, "mask_id": mask_id, "M": M, "ld": ld, "restrict": restrict and two, "modality": modality, "valid": valid,
         "zc": z.to(BF16), "zu": None, "w": None, "u": torch.rand(M, ld, generator=g, dtype=F32)}
    if guided:
        zu = torch.zeros(M, ld)
        zu[:, :V] = z[:, :V] + torch.randn(M, V, generator=g) * 0.5
        c["zu"] = zu.to(BF16)
        c["w"] = torch.where(torch.arange(M) % 3 == 0, torch.zeros(M), torch.rand(M, generator=g) * 2.0).to(F32)       # w = 0 on every third row
    return c


def poison(t, valid, V, keep_finite=False):
    """NaN in [V, ld) and, unless keep_finite (the `spikes` family: its forbidden ids hold finite +80 spikes on purpose), in every id outside `valid`"""
    p = t.clone()
    p[:, V:] = float("nan")
    if not keep_finite:
        p[:, :V] = torch.where(valid, p[:, :V], torch.full_like(p[:, :V], float("nan")))
    return p


def chi2_quantile(k, z=4.75):
    """Wilson-Hilferty: the quantile of chi-square with k degrees of freedom at the normal deviate z (z = 4.75: about 1 - 1e-6)"""
    return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


def pearson(tokens, expect_p, kept_ids):
    """(statistic, tokens outside the kept set): Pearson's X^2 of the token counts over kept_ids against expect_p (sums to 1 over kept_ids)"""
    N = tokens.numel()
    counts = torch.bincount(tokens.long(), minlength=int(kept_ids.max()) + 1)[kept_ids].double()
    outside = N - int(counts.sum())
    E = expect_p.double() * N
    return float(((counts - E) ** 2 / E).sum()), outside


CHI_V, CHI_ROWS = 96, 32768


def chi_rows():
    """three rows [CHI_V] bf16 whose nuclei hold 4, 16 and 38 ids under the batch rule with every kept p / S(n) above 2e-3 (expected counts above 60 in 32768 draws)"""
    g = torch.Generator().manual_seed(4242)
    rows = [torch.cat([torch.tensor([2.0, 1.75, 1.5, 1.25, 1.0, 0.75]), torch.full((CHI_V - 6,), -6.0)]),
            torch.cat([torch.linspace(2.0, 0.0, 24), torch.full((CHI_V - 24,), -5.0)])[torch.randperm(CHI_V, generator=g)],
            torch.cat([torch.randn(48, generator=g) * 0.3, torch.full((CHI_V - 48,), -4.0)])[torch.randperm(CHI_V, generator=g)]]
    return [r.to(BF16) for r in rows]


# the cases of tests/test_gpu_nucleus_rows.py (tests/test_nucleus_ref64.py checks on the CPU that the fp64 race alone leaves at most 1 % of their rows undecided)
# (V, Vt, mask_id, M); the valid counts are no multiples of 20, so that neither 0.855 n nor 0.95 n is an integer (the `flat` family's floor)
GPU_SHAPES = [(64, 43, 40, 300), (1000, 611, 600, 3), (4099, 3011, 3000, 1), (48385, 32001, 48384, 8)]
GPU_CASES = [(V, Vt, m, M, restrict, guided) for V, Vt, m, M in GPU_SHAPES for restrict in (False, True) for guided in (False, True)]
AR_ROWS = (1, 8, 64)


def flat_floor(ref):
    """(floor(budget n_valid) [M], clear [M]): clear where the product is further from an integer than the sums can be off (delta n_valid)"""
    x = ref.budget * ref.n_valid.double()
    fl = torch.floor(x)
    room = ref.delta * ref.n_valid.double()
    return fl.long(), ((x - fl) > room) & ((fl + 1 - x) > room)
