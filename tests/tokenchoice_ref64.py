"""fp64 reference, acceptance rule, margins and case generator for the token-choice kernels: ddpm_sample_rows_kernel (csrc/ce.hip: udm_ddpm_sample_rows,
udm_ddpm_sample_rows_cfg, udm_categorical_sample_rows) and ar_sample_rows_kernel (csrc/decode.hip: udm_ar_sample_rows).

Inputs exactly as the kernel sees them; everything after them in fp64:
    z        logits, or (1 + w) logits - w logits_uncond, every operation rounded to fp32 (nucleus_ref64.mix32)
    dt       fl32(t - s);  categorical mode: dt = 1, s = 0
    c        fl32(1e-10)
    u, g     the fp32 value the kernel loads (explicit noise) or the value of the Philox layout below
Race values
    ddpm / categorical   score_i = exp(z_i - lse) dt / (c - log(fl32(u_i + c))) over the valid ids (nucleus_ref64.valid_ids), score_mask = s / den_mask, 0 elsewhere
    greedy               z_i - lse over the valid ids; forbidden ids at -1e6, mask_id at -1e6 + its log-probability (neither can win against a valid id)
    AR                   z_i + g_i over the admissible ids
Acceptance, every row:
    the kernel's token lies in the near-maximum set {i : score_i >= max (1 - margin_row)}  (greedy, AR: {i : value_i >= max - margin_row});
    ids with bit-identical inputs (same logits bits, same u or g bits) have bit-identical kernel values: among them the lowest id must win;
    a row whose scores are all 0 (dt = 0 and s = 0) gives id 0, as torch.argmax does.
A row is decided when the near-maximum set has one element, or when all its elements are ids with bit-identical inputs ("first index").

margin_row, ddpm and categorical (relative).  The kernel holds, per id,
    score = fl(fl(e dt) / fl(c - L)),  e = exp2(fl(fl(z - lse_k) log2e)),  L = fl(log2(fl(u + c)) ln2)
  * z - lse_k rounds once: 2^-24 |z - lse| in the exponent, a factor 1 + 2^-24 A on e, with A = max |z_i - lse| over the valid ids; the product with
    log2e carries the rounding of the constant and its own: 2 * 2^-24 relative to the argument, a factor 1 + 2 * 2^-24 A.   -> 3 * 2^-24 A, taken as 4 (THETA)
  * hardware exp2: 1 ulp, 2^-23.  The product with dt: 2^-24.
  * hardware log2: 1 ulp of its result, 2^-23; the product with ln2: 2 * 2^-24.  c - L has both terms >= 0 (u + c <= 1), so the subtraction keeps the
    relative error of L and adds its own rounding: 2^-22 + 2^-24.
  * the division: unidisc_amd/csrc/Makefile compiles with -O3 and no fast-math flag, and hipcc divides fp32 correctly rounded by default: 2^-24.
  one score: 4 * 2^-24 A + (2 + 1 + 4 + 1 + 1) 2^-24;  two scores move independently:  2^-21 A + 18 * 2^-24, rounded up to
      margin = 2^-21 A + 2^-19
  The common factor exp(lse - lse_k) cancels between two ids.  It does not cancel against [MASK], whose score s / den has no lse in it: a pair (mask, id)
  carries the kernel's lse error on top, LSE_ATOL + LSE_RTOL |lse| (the bound of udm_subs_logp_rows, tests/rowops_ref64.py).
  Guided rows (w != 0): the compiler may contract the mix into a fused multiply-add, which rounds less often than mix32.  Both are within
  2 * 2^-24 B of the value with exact products, B = max (|(1 + w) z_c| + |w z_u|): z differs by at most EZ = 2^-22 B, each score by the factor exp(EZ):
  margin += 2 EZ.  A row with w = 0 mixes exactly (EZ = 0): it must equal the unguided call bit for bit.
  (An exponent argument below -126 flushes e to 0: such an id is more than 2^-126 V below the maximum and in no near-maximum set.)
margin_row, greedy (absolute): fl(z_i - lse_k) rounds once per value, 2^-24 A each:  2^-22 A + 2 EZ.
margin_row, AR with explicit g (absolute): the mix (within 2 * 2^-24 (|(1 + w) z_c| + |w z_u|) of exact, in either form) and the addition
  (2^-24 (|z| + |g|)), per value, on B_g = max (|(1 + w) z_c| + |w z_u| + |g|) over the admissible ids; two values:
      margin = 2 (n_mix + 1) 2^-24 B_g,  n_mix = 4 with guidance (2 for mix32, 2 for the kernel's form), 0 without
margin_row, AR with Philox noise: + GUMBEL_TERM, twice the worst error of the kernel's Gumbel differences measured on an MI355X against fp64 on the exact grid
  u = ((r >> 8) + 0.5) 2^-24 (tests/test_gpu_tokenchoice_rows.py::test_gumbel_error_on_the_grid measures it through the production kernel; the figure
  is in RESULTS.md).  The race only sees differences of values, so the error of a difference g_a - g_b is what is measured.

out_logp: the drawn and the `given` token within LSE_ATOL + LSE_RTOL |ref| of fp64; a `given` id that is not valid gives -inf exactly.

Philox4x32-10 (attn_prob_dropout_ref.philox4x32: key = the two halves of a 64-bit key, 64-bit counter, words x y z w):
    ddpm, categorical   key = seed;  counter = row ceil(V / 4) + (id >> 2);  word = id & 3;  u = (word >> 8) 2^-24
    AR                  key = seed ^ (step + 1) 0x9E3779B97F4A7C15 (mod 2^64);  counter = (row << 40) | (id >> 2);  word = id & 3;
                        u = ((word >> 8) + 0.5) 2^-24;  g = -log(-log(u))
Thread layout (what the `wave_ties` family aims at): column c belongs to wave (c % 256) / 64 of 4 in the ddpm kernel, and to thread (c / 8) % 512, wave
thread / 64 of 8, in the AR kernel (4096 ids per pass).
"""
import numpy as np
import torch

import nucleus_ref64 as N
from attn_prob_dropout_ref import philox4x32
from nucleus_ref64 import BF16, F32, F64, LSE_ATOL, LSE_RTOL, mix32, valid_ids

C32 = float(np.float32(1e-10))
LOG2E, LN2 = torch.tensor(1.4426950408889634, dtype=F32), torch.tensor(0.6931471805599453, dtype=F32)
GOLDEN = 0x9E3779B97F4A7C15
GUMBEL_TERM = 4.2e-6                 # twice the worst measured error of a Gumbel difference, 2.07e-6 (RESULTS.md); the GPU test asserts the measurement stays below half of it
LOGIT_FAMILIES = N.FAMILIES
FAMILIES = LOGIT_FAMILIES + ("wave_ties", "mask_wins", "near_tie", "u_edges")
M_ROWS = 64
DDPM_SHAPES = [(65, 41, 40, True), (65, 41, 20, False), (1001, 1001, 1000, False), (4099, 2051, 2050, True)]     # (V, Vt, mask_id, restrict)
AR_SHAPES = [(1000, 700, 699), (4099, 2051, 2050), (4104, 2051, 4103)]
AR_L, AR_POS, AR_STEP, AR_COL0, AR_W, AR_SEED = 12, 5, 4, 16, 1.5, 77
PHILOX_SEED = 20240229


def _arange(V):
    return torch.arange(V)[None]


def first_max(v, last=False):
    """index of the maximum per row: the first (torch.argmax, the kernels) or, for a mutant, the last"""
    V = v.shape[1]
    hit = v == v.amax(-1, keepdim=True)
    if last:
        return torch.where(hit, _arange(V), torch.full((1, 1), -1)).amax(-1)
    return torch.where(hit, _arange(V), torch.full((1, 1), V)).amin(-1)


# ------------------------------------------------------------------------------------------------ Philox on the host
def _words(key, ctr, ids):
    w = np.stack(philox4x32(key, ctr), -1)                                 # [..., 4]
    return np.take_along_axis(w, (ids & 3)[..., None].astype(np.int64), -1)[..., 0]


def philox_u_ddpm(seed, M, V, mutant=None):
    """fp32 [M, V]: the uniforms of the ddpm / categorical kernel"""
    ids = np.arange(V, dtype=np.uint64)[None]
    stride = V // 4 if mutant == "philox_row_stride" else (V + 3) // 4
    ctr = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(stride) + (ids >> np.uint64(2))
    w = _words(seed & (2 ** 64 - 1), ctr, np.broadcast_to(ids + np.uint64(1 if mutant == "philox_word_rot" else 0), ctr.shape))
    return torch.from_numpy(((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32))


def philox_x_ar(seed, step, R, V, mutant=None):
    """int64 [R, V]: word >> 8 of the AR kernel's layout"""
    key = seed & (2 ** 64 - 1)
    if mutant != "ar_key_no_step":
        key ^= ((step + 1) * GOLDEN) & (2 ** 64 - 1)
    ids = np.arange(V, dtype=np.uint64)[None]
    ctr = (np.arange(R, dtype=np.uint64)[:, None] << np.uint64(40)) | (ids >> np.uint64(2))
    w = _words(key, ctr, np.broadcast_to(ids + np.uint64(1 if mutant == "philox_word_rot" else 0), ctr.shape))
    return torch.from_numpy((w >> np.uint64(8)).astype(np.int64))


def gumbel64(x):
    """fp64 Gumbel of the grid point x = word >> 8"""
    return -torch.log(-torch.log((x.double() + 0.5) * 2.0 ** -24))


def gumbel32(x):
    """the kernel's form in torch fp32: the lower half of the grid directly, the upper half through the exact 1 - u and log1p"""
    lo = -torch.log(((x.to(F32) + 0.5) * 2.0 ** -24).to(F32))
    hi = -torch.log1p(-(((0xFFFFFF - x).to(F32) + 0.5) * 2.0 ** -24).to(F32))
    return -torch.log(torch.where(x < 2 ** 23, lo, hi))


# ------------------------------------------------------------------------------------------------ cases
def _gen(tag, family, V, guided, seed):
    return torch.Generator().manual_seed(991 + 7919 * tag + 131 * FAMILIES.index(family) + V + (17 if guided else 0) + 1000003 * seed)


def _pick(ids, g, n=1):
    return ids[torch.randperm(len(ids), generator=g)[:n]]


def _tie_rows(c, z, zu, wave_of, n_waves, g, top=3.0):
    """quantised logits below 0 and, per row, tied maxima at `top`: even rows one per wave (the lowest id not in wave 0 where that is possible), odd rows
    three in the last wave that holds valid ids; rows 0 and 1 of every four also tie the largest valid id (the ragged last stride, the AR kernel's second pass)"""
    M, V = c["M"], c["V"]
    z[:, :V] = -0.5 * torch.randint(0, 9, (M, V), generator=g).float()
    if zu is not None:
        zu[:, :V] = 0.5 * torch.randint(0, 3, (M, V), generator=g).float()
    tied = []
    for r in range(M):
        ids = c["valid"][r].nonzero()[:, 0]
        wv = wave_of(ids)
        have = sorted(set(wv.tolist()))
        if r % 2 == 0:
            pick = [int(_pick(ids[wv == k], g)) for k in have]
            if len(have) > 1 and min(pick) == pick[0]:                     # move wave 0's representative above another wave's
                later = ids[(wv == have[0]) & (ids > min(pick[1:]))]
                if len(later):
                    pick[0] = int(_pick(later, g))
        else:
            pick = _pick(ids[wv == have[-1]], g, 3).tolist()
        if r % 4 < 2:
            pick.append(int(ids[-1]))
        z[r, pick] = top
        if zu is not None:
            zu[r, pick] = 0.0
        tied.append(sorted(set(pick)))
    c["tied"] = tied


def ddpm_case(family, V, Vt, mask_id, restrict, guided, M=M_ROWS, seed=0):
    """dict: zc (zu, w) bf16 [M, ld] finite everywhere, u fp32 [M, ld] in [0, 1), t, s fp32 [M], modality, valid.  The caller poisons what the kernel must not read."""
    ld = (V + 127) // 128 * 128
    g = _gen(1, family, V, guided, seed)
    c = N.case(family if family in LOGIT_FAMILIES else "gauss", V, Vt, mask_id, M, restrict=restrict, guided=guided, seed=seed + 3, ld=ld)
    c["family"] = family
    valid = c["valid"]
    z, zu = c["zc"].float(), (c["zu"].float() if guided else None)
    u = c["u"]
    t = (0.05 + 0.95 * torch.rand(M, generator=g)).to(F32)
    s = (t * 2.0 ** -(10 + 4 * torch.rand(M, generator=g))).to(F32)       # [MASK] seldom wins: the ids race
    if family == "wave_ties":
        _tie_rows(c, z, zu, lambda ids: (ids % 256) // 64, 4, g)
        u[:] = 0.5
    elif family == "near_tie":                                             # two ids with the same logits 40 above the rest and u one ulp apart
        pairs = []
        for r in range(M):
            a, b = sorted(_pick(valid[r].nonzero()[:, 0], g, 2).tolist())
            z[r, [a, b]] = 40.0
            if guided:
                zu[r, [a, b]] = 38.0
            u[r, a], u[r, b] = 0.5, float(np.nextafter(np.float32(0.5), np.float32(1)))
            if r % 2:
                u[r, a], u[r, b] = float(u[r, b]), float(u[r, a])
            pairs.append((a, b))
        c["pairs"] = pairs
    elif family == "u_edges":
        for r in range(M):
            a, b = _pick(valid[r].nonzero()[:, 0], g, 2).tolist()
            u[r, a], u[r, b] = 0.0, 1.0 - 2.0 ** -24
    c["zc"], c["zu"] = z.to(BF16), (zu.to(BF16) if guided else None)
    if family == "mask_wins":                                              # s / den_mask = f dt max_i p_i / den_i with f = 2 (mask wins) or 1 / 2 (an id wins)
        z32 = mix32(c["zc"], c["zu"], c["w"], V).double().masked_fill(~valid, float("-inf"))
        den = C32 - torch.log((u[:, :V] + C32).double())
        best = (torch.softmax(z32, -1) / den).amax(-1)
        f = torch.where(torch.arange(M) % 2 == 0, 2.0, 0.5).double() * best * den[:, mask_id]
        s = (t.double() * f / (1 + f)).to(F32)
        s[7::8] = t[7::8]                                                  # dt = 0, s > 0: [MASK]
        t[3::8], s[3::8] = 0.0, 0.0                                        # every score 0: id 0
    c["t"], c["s"] = t, s
    return c


def ar_case(family, V, Vt, mask_id, guided, R=M_ROWS, seed=0):
    """dict as ddpm_case plus g fp32 [R, V] (explicit Gumbel noise), the modality map, x0 and x0_unmask [R, L]; restrict is always on, w is one scalar"""
    g = _gen(2, family, V, guided, seed)
    c = N.case(family if family in LOGIT_FAMILIES else "gauss", V, Vt, mask_id, R, restrict=True, guided=guided, seed=seed + 5)
    c["family"] = family
    valid = c["valid"]
    z, zu = c["zc"].float(), (c["zu"].float() if guided else None)
    if guided:
        c["w"] = torch.full((R,), AR_W, dtype=F32)
    noise = gumbel64(torch.randint(0, 2 ** 24, (R, V), generator=g)).to(F32)
    if family == "wave_ties":
        _tie_rows(c, z, zu, lambda ids: ((ids // 8) % 512) // 64, 8, g)
        noise[:] = 0.25
    elif family == "near_tie":
        pairs = []
        for r in range(R):
            a, b = sorted(_pick(valid[r].nonzero()[:, 0], g, 2).tolist())
            z[r, [a, b]] = 40.0
            if guided:
                zu[r, [a, b]] = 38.0
            noise[r, a], noise[r, b] = 1.0, float(np.nextafter(np.float32(1), np.float32(2)))
            if r % 2:
                noise[r, a], noise[r, b] = float(noise[r, b]), float(noise[r, a])
            pairs.append((a, b))
        c["pairs"] = pairs
    elif family == "u_edges":                                              # the two ends of the Gumbel grid
        for r in range(R):
            a, b = _pick(valid[r].nonzero()[:, 0], g, 2).tolist()
            noise[r, a], noise[r, b] = float(gumbel64(torch.tensor(0))), float(gumbel64(torch.tensor(2 ** 24 - 1)))
    c["zc"], c["zu"], c["g"] = z.to(BF16), (zu.to(BF16) if guided else None), noise
    mod = torch.zeros(R, AR_L, dtype=torch.int64)
    mod[:, AR_POS] = c["modality"]
    mod[:, AR_POS - 1] = 1 - c["modality"]                                 # a kernel that reads the wrong column restricts to the wrong range
    c["modmap"] = mod
    c["x0"] = torch.randint(0, V, (R, AR_L), generator=g)
    unmask = torch.zeros(R, AR_L, dtype=torch.bool)
    unmask[::3, AR_POS] = True
    unmask[:, AR_POS + 1] = True
    c["unmask"] = unmask
    return c


DDPM_FORMS = {"wave_ties": ("race", "race_cfg", "greedy", "cat"), "mask_wins": ("race", "race_cfg"), "near_tie": ("race", "cat"), "u_edges": ("race", "cat")}
AR_FORMS = {"wave_ties": ("g", "g_cfg"), "near_tie": ("g",), "u_edges": ("g",)}
PHILOX_FAMILIES = ("gauss", "flat")


def ddpm_forms(family):
    forms = DDPM_FORMS.get(family, ("race", "race_cfg", "greedy", "cat", "cat_cfg"))
    return forms + (("race_philox", "cat_philox") if family in PHILOX_FAMILIES else ())


def ar_forms(family):
    return AR_FORMS.get(family, ("g", "g_cfg", "philox", "philox_cfg"))


def ddpm_cases():
    """(shape, family, form) of every ledger row of the ddpm / categorical entry points"""
    return [(sh, f, form) for sh in DDPM_SHAPES for f in FAMILIES for form in ddpm_forms(f)]


def ar_cases():
    return [(sh, f, form) for sh in AR_SHAPES for f in FAMILIES if f != "mask_wins" for form in ar_forms(f)]


_CACHE = {}


def get_ddpm(shape, family, guided):
    k = ("ddpm", shape, family, guided)
    if k not in _CACHE:
        _CACHE[k] = ddpm_case(family, *shape, guided)
    return _CACHE[k]


def get_ar(shape, family, guided):
    k = ("ar", shape, family, guided)
    if k not in _CACHE:
        _CACHE[k] = ar_case(family, *shape, guided)
    return _CACHE[k]


def form_of(form):
    """(kind, guided, philox): kind is race / greedy / cat for ddpm, g for AR"""
    parts = form.split("_")
    philox = "philox" in parts
    return ("g" if parts[0] == "philox" else parts[0]), "cfg" in parts, philox


# ------------------------------------------------------------------------------------------------ the reference and its acceptance rule
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).long()


class Verdict:
    def __init__(self, bad, undecided, shortfall, bound, row):
        self.bad, self.undecided, self.shortfall, self.bound, self.row = bad, undecided, shortfall, bound, row


class Ref:
    """value [M, V] fp64, margin [M], relative or absolute; judge() applies the acceptance rule of the module docstring"""

    def _finish(self, c, guided, noise_bits, racing):
        V = c["V"]
        self.racing = racing                                               # ids that race by the common formula (the mask id's entry is another formula)
        self.keys = [_bits(c["zc"][:, :V])] + ([_bits(c["zu"][:, :V])] if guided else []) + ([noise_bits] if noise_bits is not None else [])
        self.top = self.value.amax(-1)
        m = self.margin[:, None].expand_as(self.value).clone()
        if self.mask_extra is not None:                                    # a pair (mask, id) carries the lse error
            mask_top = self.value[:, self.mask_id] == self.top
            m[:, self.mask_id] += self.mask_extra
            m[mask_top] += self.mask_extra[mask_top][:, None]
        self.m_id = m
        self.near = self.value >= (self.top[:, None] * (1 - m) if self.relative else self.top[:, None] - m)
        low = first_max(self.near.double())                                # the lowest id of the near-maximum set
        same = self._same(low)
        self.zero = (self.top == 0) if self.relative else torch.zeros_like(self.top, dtype=torch.bool)
        self.want = torch.where(self.zero, torch.zeros_like(low), low)
        self.decided = self.zero | (self.near.sum(-1) == 1) | ((self.near & ~same).sum(-1) == 0)

    def _same(self, tok):
        """bool [M, V]: racing ids whose inputs are bit-identical to those of tok[r] (False everywhere where tok[r] itself is not a racing id)"""
        same = self.racing & self.racing.gather(1, tok[:, None])
        for k in self.keys:
            same &= k == k.gather(1, tok[:, None])
        return same

    def judge(self, tok):
        tok = tok.long()
        M, V = self.value.shape
        bad = []
        if not bool(((tok >= 0) & (tok < V)).all()):
            return Verdict([f"token outside [0, {V})"], 0, float("inf"), 0.0, 0)
        got = self.value.gather(1, tok[:, None])[:, 0]
        short = (self.top - got) / self.top.clamp(min=1e-300) if self.relative else self.top - got
        bound = self.m_id.gather(1, tok[:, None])[:, 0]
        outside = ~self.near.gather(1, tok[:, None])[:, 0] & ~self.zero
        if bool(outside.any()):
            r = int(outside.nonzero()[0])
            bad.append(f"{int(outside.sum())} rows with a token outside the near-maximum set, first row {r}: {int(tok[r])} (short by {float(short[r]):.3e}, "
                       f"margin {float(bound[r]):.3e}), exact {int(self.want[r])}")
        first = first_max(self._same(tok).double())
        twin = self._same(tok).any(-1) & (first != tok) & ~self.zero
        if bool(twin.any()):
            r = int(twin.nonzero()[0])
            bad.append(f"{int(twin.sum())} rows where a bit-identical lower id lost, first row {r}: {int(tok[r])} instead of {int(first[r])}")
        z = self.zero & (tok != 0)
        if bool(z.any()):
            bad.append(f"{int(z.sum())} all-zero rows without id 0, first row {int(z.nonzero()[0])}")
        ratio = torch.where(self.zero, torch.zeros_like(short), short / bound.clamp(min=1e-300))
        r = int(ratio.argmax())
        return Verdict(bad, int((~self.decided).sum()), float(short[r]) if not bool(self.zero[r]) else 0.0, float(bound[r]), r)


def _mix_error(c, guided, valid, extra=None):
    """(EZ [M], B [M]): the bound on the kernel's z against mix32, and max (|(1 + w) z_c| + |w z_u| (+ |extra|)) over `valid`"""
    V = c["V"]
    zc = c["zc"][:, :V].double()
    if guided:
        w = c["w"].double()[:, None]
        b = ((1 + w) * zc).abs() + (w * c["zu"][:, :V].double()).abs()
    else:
        b = zc.abs()
    B = b.masked_fill(~valid, 0.0).amax(-1)
    Bx = (b + (extra.abs() if extra is not None else 0.0)).masked_fill(~valid, 0.0).amax(-1)
    EZ = torch.where(c["w"] == 0, 0.0, 2.0 ** -22).double() * B if guided else torch.zeros_like(B)
    return EZ, Bx


class DdpmRef(Ref):
    def __init__(self, c, form, u=None):
        kind, guided, _ = form_of(form)
        M, V, valid = c["M"], c["V"], c["valid"]
        self.mask_id, self.kind = c["mask_id"], kind
        self.z32 = mix32(c["zc"], c["zu"] if guided else None, c["w"] if guided else None, V)
        z = self.z32.double()
        zm = z.masked_fill(~valid, float("-inf"))
        self.lse = torch.logsumexp(zm, -1)
        self.logp = zm - self.lse[:, None]                                 # -inf on every id that is not valid
        A = self.logp.masked_fill(~valid, 0.0).abs().amax(-1)
        EZ, _ = _mix_error(c, guided, valid)
        self.lse_tol = LSE_ATOL + LSE_RTOL * self.lse.abs()
        if kind == "greedy":
            self.value = torch.where(valid, self.logp, torch.full_like(z, -1e6))
            self.value[:, self.mask_id] = -1e6 + (z[:, self.mask_id] - self.lse)
            self.margin, self.relative, self.mask_extra = 2.0 ** -22 * A + 2 * EZ, False, None
            self._finish(c, guided, None, valid)
            return
        self.u = (c["u"] if u is None else u)[:, :V].to(F32)
        dt, s = (torch.ones(M, dtype=F64), torch.zeros(M, dtype=F64)) if kind == "cat" else ((c["t"] - c["s"]).double(), c["s"].double())
        den = C32 - torch.log((self.u + C32).double())
        self.value = torch.where(valid, torch.exp(self.logp) * dt[:, None] / den, torch.zeros_like(z))
        self.value[:, self.mask_id] = s / den[:, self.mask_id]
        self.margin, self.relative, self.mask_extra = 2.0 ** -21 * A + 2.0 ** -19 + 2 * EZ, True, self.lse_tol
        self._finish(c, guided, _bits(self.u), valid)

    def logp_ok(self, tok, logp):
        """(bool [M], worst error): out_logp against fp64; -inf exactly for an id that is not valid"""
        want = self.logp.gather(1, tok.long()[:, None])[:, 0]
        fin = torch.isfinite(want)
        err = torch.where(fin, (logp.double() - want).abs(), torch.zeros_like(want))
        ok = torch.where(fin, err <= LSE_ATOL + LSE_RTOL * want.abs(), logp.double() == float("-inf"))
        return ok, float(err.max())


class ArRef(Ref):
    def __init__(self, c, form, x=None):
        """x: int64 [R, V] Philox grid points (word >> 8) for the philox forms; the explicit c["g"] otherwise"""
        _, guided, philox = form_of(form)
        V, valid = c["V"], c["valid"]
        self.mask_id = c["mask_id"]
        self.z32 = mix32(c["zc"], c["zu"] if guided else None, c["w"] if guided else None, V)
        g = gumbel64(x) if philox else c["g"].double()
        self.value = (self.z32.double() + g).masked_fill(~valid, float("-inf"))
        _, Bg = _mix_error(c, guided, valid, extra=g)
        self.margin = 2 * ((4 if guided else 0) + 1) * 2.0 ** -24 * Bg + (GUMBEL_TERM if philox else 0.0)
        self.relative, self.mask_extra = False, None
        self._finish(c, guided, x if philox else _bits(c["g"]), valid)


def writeback(c, tok, guided, mutant=None):
    """(x[:, pos] [R], next_ids [R] or [2 R]) of the AR kernel after choosing tok"""
    keep = c["unmask"][:, AR_POS]
    val = torch.where(keep, c["x0"][:, AR_POS], tok.long())
    if not guided:
        return val, val.clone()
    un = val if mutant == "ar_next_ids_unmasked" else torch.where(keep, torch.full_like(val, c["mask_id"]), val)
    return val, torch.cat([val, un])


def ddpm_ref(shape, family, form):
    """the case and its reference, computed once and shared (the philox forms: the host's uniforms at PHILOX_SEED)"""
    k = ("ddpm_ref", shape, family, form)
    if k not in _CACHE:
        kind, guided, philox = form_of(form)
        c = get_ddpm(shape, family, guided)
        _CACHE[k] = (c, DdpmRef(c, form, philox_u_ddpm(PHILOX_SEED, c["M"], c["V"]) if philox else None))
    return _CACHE[k]


def ar_ref(shape, family, form):
    k = ("ar_ref", shape, family, form)
    if k not in _CACHE:
        _, guided, philox = form_of(form)
        c = get_ar(shape, family, guided)
        _CACHE[k] = (c, ArRef(c, form, philox_x_ar(AR_SEED, AR_STEP, c["M"], c["V"]) if philox else None))
    return _CACHE[k]


def violations_ddpm(shape, family, form, tok, logp=None):
    """(list of violations, Verdict): the race rule, the undecided count the family promises, and for the categorical forms out_logp"""
    c, ref = ddpm_ref(shape, family, form)
    v = ref.judge(tok)
    bad = list(v.bad)
    if family == "near_tie":
        if v.undecided != c["M"]:
            bad.append(f"{c['M'] - v.undecided} near_tie rows decided")
        if not all(int(tok[r]) in c["pairs"][r] for r in range(c["M"])):
            bad.append("a near_tie token outside its pair")
    elif v.undecided:
        bad.append(f"{v.undecided} undecided rows")
    if logp is not None and form_of(form)[0] == "cat":
        ok, err = ref.logp_ok(tok, logp)
        if not bool(ok.all()):
            bad.append(f"out_logp off by {err:.3e} in {int((~ok).sum())} rows")
    return bad, v


def violations_ar(shape, family, form, tok, xcol=None, next_ids=None):
    c, ref = ar_ref(shape, family, form)
    v = ref.judge(tok)
    bad = list(v.bad)
    if family == "near_tie":
        if v.undecided != c["M"]:
            bad.append(f"{c['M'] - v.undecided} near_tie rows decided")
        if not all(int(tok[r]) in c["pairs"][r] for r in range(c["M"])):
            bad.append("a near_tie token outside its pair")
    elif v.undecided:
        bad.append(f"{v.undecided} undecided rows")
    if xcol is not None:
        wx, wn = writeback(c, tok, form_of(form)[1])
        if not torch.equal(xcol, wx):
            bad.append("x[:, pos] is not where(x0_unmask, x0, token)")
        if not torch.equal(next_ids, wn):
            bad.append("next_ids is not (x[:, pos], where(x0_unmask, mask_id, x[:, pos]))")
    return bad, v


# ------------------------------------------------------------------------------------------------ fp32 emulations and mutants
DDPM_MUTANTS = ("last_index", "mask_admitted", "other_modality", "q_mask_dropped", "dt_is_t", "lse_all_columns", "w_wrong_row", "mix_bf16", "philox_word_rot",
                "philox_row_stride")
AR_MUTANTS = ("last_index", "mask_admitted", "other_modality", "mix_bf16", "philox_word_rot", "ar_key_no_step", "ar_next_ids_unmasked")


def _mutant_inputs(c, guided, mutant):
    """(z fp32 [M, V], valid) under the mutant"""
    M, V = c["M"], c["V"]
    w = c["w"] if guided else None
    if mutant == "w_wrong_row" and guided:
        w = torch.roll(w, 1)
    z = mix32(c["zc"], c["zu"] if guided else None, w, V)
    if mutant == "mix_bf16":
        z = z.to(BF16).to(F32)
    valid = valid_ids(M, V, c["Vt"], c["mask_id"], c["modality"], c["restrict"] and mutant != "other_modality",
                      mutant="forbidden_kept" if mutant == "mask_admitted" else None)
    return z, valid


def _lse_lanes(zm, lanes=256):
    """fp32 lse as the kernel builds it: per strided lane a maximum and a sum of exp2((z - m) log2e), then a pairwise tree over the lanes"""
    M, V = zm.shape
    pad = (V + lanes - 1) // lanes * lanes
    zp = torch.full((M, pad), float("-inf"), dtype=F32)
    zp[:, :V] = zm
    zp = zp.view(M, pad // lanes, lanes)
    m = zp.amax(1)
    s = torch.where(torch.isfinite(zp), torch.exp2((zp - torch.where(torch.isfinite(m), m, torch.zeros_like(m))[:, None]) * LOG2E), torch.zeros_like(zp)).sum(1)
    n = lanes
    while n > 1:
        n //= 2
        m1, m2, s1, s2 = m[:, :n], m[:, n:2 * n], s[:, :n], s[:, n:2 * n]
        mm = torch.maximum(m1, m2)
        safe = torch.where(torch.isfinite(mm), mm, torch.zeros_like(mm))
        s = torch.where(torch.isfinite(m1), s1 * torch.exp2((m1 - safe) * LOG2E), torch.zeros_like(s1)) + \
            torch.where(torch.isfinite(m2), s2 * torch.exp2((m2 - safe) * LOG2E), torch.zeros_like(s2))
        m = mm
    return m[:, 0] + torch.log2(s[:, 0]) * LN2


def _tree_argmax(v, thread_of, n_threads, last=False):
    """argmax as the kernels run it: every thread keeps the first maximum of its own ids, then a pairwise tree with (value, lower id) as the order"""
    M, V = v.shape
    th = thread_of(torch.arange(V))
    bv = torch.full((M, n_threads), float("-inf"), dtype=v.dtype)
    bi = torch.full((M, n_threads), 2 ** 62, dtype=torch.int64)
    for k in range(n_threads):
        cols = (th == k).nonzero()[:, 0]
        if len(cols):
            sub = v[:, cols]
            j = first_max(sub, last)
            ok = ~torch.isnan(sub.gather(1, j.clamp(0, len(cols) - 1)[:, None])[:, 0]) & (sub.amax(-1) > float("-inf"))
            bv[:, k] = torch.where(ok, sub.amax(-1), bv[:, k])
            bi[:, k] = torch.where(ok, cols[j.clamp(0, len(cols) - 1)], bi[:, k])
    n = n_threads
    while n > 1:
        n //= 2
        v1, v2, i1, i2 = bv[:, :n], bv[:, n:2 * n], bi[:, :n], bi[:, n:2 * n]
        take2 = (v2 > v1) | ((v2 == v1) & ((i2 > i1) if last else (i2 < i1)))
        bv, bi = torch.where(take2, v2, v1), torch.where(take2, i2, i1)
    return bi[:, 0]


def emulate_ddpm(c, form, arith="torch32", mutant=None, seed=PHILOX_SEED):
    """(token [M], log p(token) [M] fp32) of an fp32 implementation.  arith: "torch32" (exp / log, one argmax, as tests/fake_kernels.py) or "lanes32" (exp2 / log2
    scaled, 256 strided lanes, tree-reduced)."""
    kind, guided, philox = form_of(form)
    M, V, mask_id = c["M"], c["V"], c["mask_id"]
    z, valid = _mutant_inputs(c, guided, mutant)
    zm = z.masked_fill(~valid, float("-inf"))
    over = z if mutant == "lse_all_columns" else zm
    lse = torch.logsumexp(over, -1) if arith == "torch32" else _lse_lanes(over)
    logp = zm - lse[:, None]
    last = mutant == "last_index"
    pick = (lambda v: first_max(v, last)) if arith == "torch32" else (lambda v: _tree_argmax(v, lambda i: i % 256, 256, last))
    if kind == "greedy":
        score = torch.where(valid, logp, torch.full_like(logp, -1e6))
        if mutant != "mask_admitted":
            score[:, mask_id] = -1e6 + z[:, mask_id] - lse
        tok = pick(score)
        return tok, logp.gather(1, tok[:, None])[:, 0]
    u = philox_u_ddpm(seed, M, V, mutant) if philox else c["u"][:, :V]
    if kind == "cat":
        dt, s = torch.ones(M, dtype=F32), torch.zeros(M, dtype=F32)
    else:
        dt, s = (c["t"] if mutant == "dt_is_t" else c["t"] - c["s"]), c["s"]
    if arith == "torch32":
        q = torch.where(valid, logp.exp() * dt[:, None], torch.zeros_like(logp))
        den = C32 - (u + C32).log()
    else:
        q = torch.where(valid, torch.exp2(logp * LOG2E) * dt[:, None], torch.zeros_like(logp))
        den = C32 - torch.log2(u + C32) * LN2
    if mutant != "mask_admitted":
        q[:, mask_id] = 0.0 if mutant == "q_mask_dropped" else s
    tok = pick(q / den)
    return tok, logp.gather(1, tok[:, None])[:, 0]


def emulate_ar(c, form, arith="torch32", mutant=None, seed=AR_SEED, step=AR_STEP):
    """(token [R], x[:, pos], next_ids) of an fp32 implementation.  arith: "torch32" (one argmax) or "lanes32" (512 threads of 8 consecutive ids, tree-reduced)"""
    _, guided, philox = form_of(form)
    R, V = c["M"], c["V"]
    z, valid = _mutant_inputs(c, guided, mutant)
    g = gumbel32(philox_x_ar(seed, step, R, V, mutant)) if philox else c["g"]
    v = (z + g).masked_fill(~valid, float("-inf"))
    last = mutant == "last_index"
    tok = first_max(v, last) if arith == "torch32" else _tree_argmax(v, lambda i: (i // 8) % 512, 512, last)
    return (tok,) + writeback(c, tok, guided, mutant)
