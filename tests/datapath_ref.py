"""Serial and fp64 statements of the kernels that build a training batch before the first GEMM and turn log-probabilities into the loss after the last one -
udm_assemble_joint_tokens, udm_sample_t_noise, udm_qxt_absorbing, udm_interleaved_rope, udm_interleaved_block_lottery (csrc/tokens.hip),
udm_attention_doc_ranges (csrc/attention.hip), udm_diffusion_loss (csrc/ce.hip) - with their input families, bounds, judges and mutants (CPU only; nothing of
the product is imported here, but for the mask-code inputs of doc_code_cases, which take the modality codes from kernels.modality_mask_codes, plain torch).

The reference of tests/test_gpu_datapath_exact.py (GPU) and the subject of tests/test_datapath_ref.py (CPU); the split follows smallops_ref64.py.

Serial statements (`*_ref`): Python loops over rows and positions on numpy arrays, written from the comments at the top of the kernels - no cummax, no sort, no
scatter.  Everything integer or bool is judged exactly (`same`).  Preconditions of the packed-row kernels (include/unidisc_hip.h): -1 is the only negative
sample id, and ids are below L (the packing collate numbers the samples of a row 0, 1, 2 ..); the families respect both.

udm_sample_t_noise, two statements.  (1) `t_noise_ieee`: the kernel's operations in numpy fp32, one correctly rounded operation each (contraction is off in
the kernel): inv_n = fl(1 / fl(n)), off = fl(i) inv_n, e = fmod(fl(fl(u inv_n) + off), 1), t = fl(fl(c e) + eps), den = fl(1 - fl(c' t)),
dsigma = fl(fl(1 / den) c') - t and dsigma are asserted bit for bit.  (2) fp64 at the kernel's own t: sigma64 = -log1p(-c' t), move64 = 1 - exp(-sigma64) =
c' t; the device log1pf / expf are not correctly rounded, so
    sigma   E = FACTOR W 2^-24 (sigma64 + c' t / (1 - c' t))                  (the argument's rounding, amplified by d sigma / d arg, and log1p's own)
    move    E = FACTOR W 2^-24 (move64 + (1 - move64) (1 + sigma64) + c' t)   (sigma's error times exp(-sigma), exp's own, the subtraction)
FACTOR = 4 as in smallops_ref64; W is the worst ratio the fp32 restatement in torch CPU ops (`t_noise_f32`, the kernel's order) reaches against fp64 at
FACTOR W = 1, rounded up: W_SIGMA = 1 (measured 0.957), W_MOVE = 1 (measured 0.792); tests/test_datapath_ref.py measures both again.

udm_diffusion_loss.  `loss_ref`: fp64 from the fp32 inputs with the kernel's conventions (an empty modality contributes 0 and passes no gradient, 0 / 0 gives
loss 0; the fractions are NaN when no attended token has a modality).  nlls is one fp32 product: exact.  Counts are exact, fractions within one rounding.
Sums: all terms are non-negative (-log_p >= 0, w >= 0 in the families), so a chain of k roundings gives |got - ref| <= gamma_k ref, gamma_k = k u / (1 - k u),
u = 2^-24.  `sum_chain(N)` = 1 (the term's product; 0 if contracted into an FMA) + ceil(N / 1024) (serial additions of a thread) + 6 (wave tree) + 16 (block
sum) = ceil(N / 1024) + 23.  `loss_bound(N, case)` adds the roundings of the kernel's expressions:
    mean            loss k + 1 (the division);   coef 2 (1 / n, the product with -w)
    weighted        txt_loss, img_loss k + 4 (division, the fraction, two products);   loss k + 5;   coef 6 (fraction, two products, division, a sum when a token
                    has both modalities, the product with -w)
    cap active      scale = (ratio img) / (txt + 1e-8): 2 (k + 4) + 3;  txt_loss 3 (k + 4) + 4;  loss one more;  coef 6 + 2 (k + 4) + 3
The capped families keep the fp64 ratio at least 1e-3 away from 1, so fp32 and fp64 take the same side of the min.
"""
import numpy as np
import torch

F32N, F64N = np.float32, np.float64
U = 2.0 ** -24
FACTOR = 4
W_SIGMA, W_MOVE = 1, 1
W_MEASURED = dict(sigma=0.957, move=0.792)
SEPS, NEPS = 1e-3, 1e-3                      # sampling_eps, the schedule's eps
LENGTHS = (1, 4, 5, 255, 256, 257, 300, 777, 1536)
SIZES = {0: (), 1: (16,), 8: (4, 16, 64, 1, 7, 100, 32, 2)}
ROPE_CONFIGS = ((0, 4), (1, 4), (8, 16))     # (nsizes, half)
TXT_ROWS = 40
MASK_PROBS = (0.0, 0.2, 0.9)
T_NOISE_N = (1, 2, 3, 7, 64, 100, 255, 256, 257, 4099)
QXT_SHAPES = ((1, 1), (3, 255), (3, 256), (3, 257), (64, 333))
QXT_DRAWS = ("none", "txt", "img", "both")
ASSEMBLE_SHAPES = ((0, 5), (5, 0), (3, 254), (128, 1024), (100, 157))
DOC_SHAPES = ((1, 1), (2, 64), (3, 200), (2, 130), (1, 257))
LOSS_SHAPES = ((1, 1), (1, 1023), (1, 1024), (5, 205), (6, 200), (8, 4608))
LOSS_CASES = ("weighted", "weighted_cap", "weighted_no_image", "mean", "mean_full_mask", "mean_no_modality", "all_padding", "cap_active", "cap_inactive", "cap_zero",
              "neither_modality")
MUTANTS = ("runs_split_at_id", "cand_ge4", "k_not_k1", "n_over_row", "rank_per_row", "j_over_row", "txt_from_row_start", "qxt_le", "qxt_both_masks_both",
           "offset_i_plus_1", "doc_hi_off_by_one", "doc_exact_ignores_foreign", "doc_span_on_whole_code", "doc_class_bits_are_not_padding", "mean_counts_unattended", "cap_on_image", "coef_without_fraction")


def _rng(seed):
    return np.random.default_rng(int(seed))


def f32(v):
    return float(F32N(v))


def same(got, ref):
    """number of elements that differ by value (NaN equals NaN, +0 equals -0) - the exact judge of everything integer, bool, t, dsigma and nlls"""
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    bad = g != r
    if g.dtype.kind == "f":
        bad &= ~(np.isnan(g) & np.isnan(r))
    return int(bad.sum())


def ratio(got, ref, E):
    """largest |got - ref| / E over the elements (0 where got == ref; inf for a NaN or a missed zero bound): the bounded judge, every element"""
    g, r, E = np.asarray(got, F64N), np.asarray(ref, F64N), np.broadcast_to(np.asarray(E, F64N), np.shape(ref))
    with np.errstate(all="ignore"):
        err = np.abs(g - r)
        q = np.where(err == 0, 0.0, err / E)
    q = np.where(np.isnan(g) & np.isnan(r), 0.0, q)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ joint assembly
def assemble_ref(txt, txt_mask, img, idx, B, Vt):
    """(ids int64, mask bool, modality int64) [B, Lt + Li]: row b gathers dataset row idx[b] (b without idx); text ids widen, image ids widen WITH their sign
    and shift by Vt; the mask is the text mask (all valid without one) and 1 on the image positions"""
    Lt, Li = txt.shape[1], img.shape[1]
    ids, mask, mod = np.zeros((B, Lt + Li), np.int64), np.zeros((B, Lt + Li), bool), np.zeros((B, Lt + Li), np.int64)
    for b in range(B):
        row = int(idx[b]) if idx is not None else b
        for l in range(Lt + Li):
            if l < Lt:
                ids[b, l], mask[b, l], mod[b, l] = int(txt[row, l]), (True if txt_mask is None else bool(txt_mask[row, l])), 0
            else:
                ids[b, l], mask[b, l], mod[b, l] = int(img[row, l - Lt]) + Vt, True, 1
    return ids, mask, mod


def assemble_cases():
    out = []
    for k, (Lt, Li) in enumerate(ASSEMBLE_SHAPES):
        g = _rng(100 + k)
        n = 7
        txt = g.integers(-5, 30000, (n, Lt)).astype(np.int32)
        img = g.integers(-32768, 32768, (n, Li)).astype(np.int16)
        if Li:
            img[0, 0], img[n - 1, Li - 1] = -32768, -1
        tm = g.random((n, Lt)) < 0.8
        for name, idx, mask in (("plain", None, tm), ("permuted", g.permutation(n).astype(np.int64), tm), ("repeats", np.array([3, 3, 0, 6, 3, 6, 1, 0, 2, 5, 4], np.int64), tm),
                                ("no_mask", np.array([6, 0], np.int64), None)):
            out.append(dict(name=f"Lt{Lt}-Li{Li}-{name}", txt=txt, txt_mask=mask, img=img, idx=idx, B=n if idx is None else len(idx), Vt=30001))
    return out


# ------------------------------------------------------------------------------------------------ absorbing mask
def qxt_ref(x, r_move, mc, r_txt, r_img, thr_txt, thr_img, mm, mask_id, mutant=None):
    """(xt, move [B, L], row_txt, row_img, row_ignore [B]): move = r_move < mc[b]; a row drawn for exactly one modality REPLACES its move by that modality's
    columns, a row drawn for both keeps its per-token move; xt = move ? mask_id : x.  Strict comparisons on fp32 values."""
    B, L = x.shape
    lt = (lambda a, b: a <= b) if mutant == "qxt_le" else (lambda a, b: a < b)
    xt, move = x.copy(), np.zeros((B, L), bool)
    rows = np.zeros((3, B), bool)
    for b in range(B):
        mt = r_txt is not None and bool(lt(F32N(r_txt[b]), F32N(thr_txt)))
        mi = r_img is not None and bool(lt(F32N(r_img[b]), F32N(thr_img)))
        if mt and mi and mutant != "qxt_both_masks_both":
            mt = mi = False
        rows[:, b] = mt, mi, mt or mi
        for l in range(L):
            mv = bool(lt(F32N(r_move[b, l]), F32N(mc[b])))
            if mt and mi:
                mv = bool(mm[b, l, 0]) or bool(mm[b, l, 1])
            elif mt:
                mv = bool(mm[b, l, 0])
            elif mi:
                mv = bool(mm[b, l, 1])
            move[b, l] = mv
            if mv:
                xt[b, l] = mask_id
    return xt, move, rows[0], rows[1], rows[2]


def qxt_cases():
    """every shape x draw mode: r_move == move_chance on a few positions, row 0 exactly on the threshold (not drawn), row 1 - where there is one - drawn for both
    modalities, the last row just below the threshold (drawn)"""
    out = []
    for B, L in QXT_SHAPES:
        for draws in QXT_DRAWS:
            g = _rng(B * 1000 + L + len(draws))
            p = 0.3
            x = g.integers(0, 4000, (B, L)).astype(np.int64)
            r_move, mc = g.random((B, L), F32N), g.random(B, F32N)
            r_move[B // 2, : min(L, 7)] = mc[B // 2]
            r_move[0, L - 1] = mc[0]
            mm = np.zeros((B, L, 2), bool)
            mm[:, : L // 3, 0] = True
            mm[:, L // 3 + (1 if L > 4 else 0):, 1] = True        # from L = 5 on one position of neither modality
            p_txt, p_img = (p, 0.0) if draws == "txt" else (0.0, p) if draws == "img" else (p / 2, p / 2)
            thr_t, thr_i = F32N(p_txt), F32N(p_img)
            r_txt = g.random(B, F32N) if draws in ("txt", "both") else None
            r_img = g.random(B, F32N) if draws in ("img", "both") else None
            for r, thr in ((r_txt, thr_t), (r_img, thr_i)):
                if r is not None:
                    r[0] = thr
                    r[B - 1] = np.nextafter(thr, F32N(0)) if B > 1 else thr
                    if B > 2:
                        r[1] = 0.0
                        r[2] = 0.0 if r is r_txt else 0.9
            out.append(dict(name=f"B{B}-L{L}-{draws}", x=x, r_move=r_move, mc=mc, r_txt=r_txt, r_img=r_img, thr_txt=thr_t, thr_img=thr_i, p_txt=p_txt, p_img=p_img,
                            mm=mm, mask_id=4242))
    return out


# ------------------------------------------------------------------------------------------------ document ranges
def code_id(code):
    """the id field of a mask code: its low 32 bits, sign-extended"""
    return ((int(code) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def doc_ranges_ref(sid, mutant=None):
    """int32 [B, ceil(L / 64), 8]: per 64-row tile {lo, hi, idmin, idmax, exact, 0, 0, 0}.  `sid` holds mask codes (csrc/attention_common.h); the id of a position
    is the sign-extended low 32 bits of its code, id < 0 is padding.  [idmin', idmax'] = the interval of the tile's ids >= 0; [lo, hi) spans the row's positions
    whose ID lies inside it; idmin = -1 when the tile holds padding OR any position with a bit above bit 31 set (class bits); ids >= 2^30 are never reported
    (idmin = -1, idmax = -2); exact = one document, no padding, no class bits, and every position of [lo, hi) holds it without class bits.  A tile without any
    id >= 0: {0, 0, -1, -2, 0}.  Rows past L are not padding.  For raw ids in [-2^31, 2^31) this is the definition on the whole value."""
    B, L = sid.shape
    nT = (L + 63) // 64
    out = np.zeros((B, nT, 8), np.int32)
    whole = mutant == "doc_span_on_whole_code"
    ident = (lambda c: c) if whole else code_id
    for b in range(B):
        row = [int(v) for v in sid[b]]
        for t in range(nT):
            tile = row[t * 64:min(t * 64 + 64, L)]
            ids = [ident(c) for c in tile if ident(c) >= 0]
            if not ids:
                out[b, t, :5] = 0, 0, -1, -2, 0
                continue
            high = any(c >> 32 != 0 for c in tile) and not whole and mutant != "doc_class_bits_are_not_padding"
            mn, mx, pad = min(ids), max(ids), len(ids) < len(tile) or high
            hits = [j for j in range(L) if mn <= ident(row[j]) <= mx]
            lo, hi = hits[0], hits[-1] + 1
            small = mx < 2 ** 30
            idmin, idmax = (mn if small and not pad else -1), (mx if small else -2)
            clean = len(hits) if whole else sum(1 for j in hits if row[j] >> 32 == 0)
            full = clean == hi - lo or mutant == "doc_exact_ignores_foreign"
            out[b, t, :5] = lo, hi + (1 if mutant == "doc_hi_off_by_one" else 0), idmin, idmax, int(idmin >= 0 and idmin == idmax and full)
    return out


def doc_cases():
    out = []
    for B, L in DOC_SHAPES:
        g = _rng(7 * B + L)
        sid = np.full((B, L), -1, np.int64)
        for b in range(B):
            pos, s = 0, 0
            while pos < L - (b % 2) * (L // 5):
                n = int(g.integers(1, 90))
                sid[b, pos:pos + n] = s
                pos, s = pos + n, s + 1
        if L >= 200 and B >= 3:
            sid[0, :64], sid[0, 64:100], sid[0, 100:128], sid[0, 128:] = 3, 5, 3, 4          # tile 0 holds one document that comes back behind a foreign one
            sid[1, :] = 2 ** 30 + 7                                                             # ids that do not fit
            sid[1, 64:128] = 2 ** 30 - 1
            sid[2, :64], sid[2, 64:128], sid[2, 128:] = 0, -1, 0                                # an all-padding tile between two of one document
            sid[2, 10] = -1                                                                     # padding inside a tile
        out.append(dict(name=f"B{B}-L{L}", sid=sid))
    return out + doc_code_cases()


DOC_RAW_CASES = len(DOC_SHAPES)      # doc_cases()[:DOC_RAW_CASES] hold raw ids only


def doc_code_cases():
    """mask codes (class bits above the id field): the layouts of attention_ref64.code_layouts at L = 320 - the modality codes come from the product's
    modality_mask_codes, plain torch - and one row set whose codes have an id field of -1 (0xFFFFFFFF) under positive class bits, padding under a key mask"""
    import attention_ref64 as R

    B, L = 4, 320
    out = []
    for Lt in (72, 128):
        for name, codes in R.code_layouts(B, L, Lt).items():
            if Lt == 72 or name.startswith("modality"):
                out.append(dict(name=f"codes-{name}-Lt{Lt}", sid=codes.numpy().copy()))
    cls = (1 << 32) | (3 << 40)
    sid = np.zeros((3, 200), np.int64)
    sid[0, :] = cls                                   # sample 0 with class bits everywhere ...
    sid[0, 70:140] = 0xFFFFFFFF | (4 << 32) | (3 << 40)   # ... and padding under a masked key, across the seam of tiles 1 and 2
    sid[1, :64], sid[1, 64:128], sid[1, 128:] = 0xFFFFFFFF | cls, 1, 1 | cls      # a tile of coded padding only, a raw tile, the same document with class bits
    sid[2, :100], sid[2, 100:] = 0, 1                 # raw documents ...
    sid[2, 192:] = 0xFFFFFFFF | cls                   # ... and coded padding in the ragged last tile
    out.append(dict(name="codes-padding-under-class-bits", sid=sid))
    return out


# ------------------------------------------------------------------------------------------------ interleaved rope
def rope_ref(mod, sid, sizes, txt_rows, mutant=None):
    """per position (src, row, cidx): src 1 = image table row `row` (the tables of `sizes` concatenated), 2 = text table row `row`, 0 = zeros; cidx the image-count
    index or -1.  Also the image-run starts of every row (the scratch contract)."""
    B, L = mod.shape
    src, row, cidx, starts = np.zeros((B, L), np.int64), np.full((B, L), -1, np.int64), np.full((B, L), -1, np.int64), []
    for b in range(B):
        seen, l = [], 0                                          # sample ids of the image-run starts so far
        while l < L:
            if mod[b, l] == 0:
                l += 1
                continue
            e = l + 1
            while e < L and mod[b, e] != 0 and not (mutant == "runs_split_at_id" and sid[b, e] != sid[b, e - 1]):
                e += 1
            j = len(seen) if mutant == "j_over_row" else sum(1 for s in seen if s == sid[b, l])
            seen.append(int(sid[b, l]))
            starts.append((b, l))
            if (e - l) in sizes:
                base = sum(sizes[:sizes.index(e - l)])
                for q in range(l, e):
                    src[b, q], row[b, q], cidx[b, q] = 1, base + q - l, j
            l = e
        ss = 0
        for l in range(L):
            if l == 0 or sid[b, l] != sid[b, l - 1]:
                ss = l                                            # start of the run of constant sample id (whatever the modality)
            if mod[b, l] == 0 and sid[b, l] >= 0:
                src[b, l], row[b, l] = 2, min(l - (0 if mutant == "txt_from_row_start" else ss), txt_rows - 1)
    return src, row, cidx, [[l for bb, l in starts if bb == b] for b in range(B)]


def rope_tables(nsizes, half, seed=0):
    """(sizes, img_cos, img_sin [max(sum sizes, 1), half], txt_cos, txt_sin [TXT_ROWS, half]) fp32, every entry different"""
    g = _rng(900 + nsizes + half + seed)
    sizes = SIZES[nsizes]
    rows = max(sum(sizes), 1)
    return sizes, g.standard_normal((rows, half)).astype(F32N), g.standard_normal((rows, half)).astype(F32N), g.standard_normal((TXT_ROWS, half)).astype(F32N), \
        g.standard_normal((TXT_ROWS, half)).astype(F32N)


def rope_apply(src, row, img_t, txt_t):
    """the table rows the statement names, fp32 [B, L, half]"""
    out = np.zeros(src.shape + (img_t.shape[1],), F32N)
    out[src == 1] = img_t[row[src == 1]]
    out[src == 2] = txt_t[row[src == 2]]
    return out


# ------------------------------------------------------------------------------------------------ block lottery
def lottery_ref(mod, sid, r, n_r, mask_prob, mutant=None):
    """(accum bool [B, L], rows_hit bool [B], n_cand, thresholds fp32 [n_cand], candidate starts per row).  Blocks = runs of constant (modality, id); a candidate
    has id >= 0 and more than 4 tokens; rank counts candidates in (row, position) order over the batch; k / n over the candidates of (row, id)."""
    B, L = mod.shape
    accum, rows_hit, rank, thrs, cstarts = np.zeros((B, L), bool), np.zeros(B, bool), 0, [], []
    p = F32N(mask_prob)
    for b in range(B):
        blocks, l = [], 0
        while l < L:
            e = l + 1
            while e < L and mod[b, e] == mod[b, l] and sid[b, e] == sid[b, l]:
                e += 1
            blocks.append((l, e))
            l = e
        cands = [(s, e) for s, e in blocks if sid[b, s] >= 0 and (e - s >= 4 if mutant == "cand_ge4" else e - s > 4)]
        cstarts.append([s for s, _ in cands])
        if mutant == "rank_per_row":
            rank = 0
        for q, (s, e) in enumerate(cands):
            mates = [i for i, (s2, _) in enumerate(cands) if sid[b, s2] == sid[b, s]]
            k, n = mates.index(q), (len(cands) if mutant == "n_over_row" else len(mates))
            thr = F32N(F32N(p * F32N(F32N(k if mutant == "k_not_k1" else k + 1) / F32N(n))) * F32N(2))
            thrs.append(thr)
            if rank < n_r and F32N(r[rank]) < thr:
                accum[b, s:e], rows_hit[b] = True, True
            rank += 1
    n_cand = rank if mutant != "rank_per_row" else sum(len(c) for c in cstarts)
    return accum, rows_hit, n_cand, np.array(thrs, F32N), cstarts


def lottery_uniforms(mod, sid, mask_prob, n_r, seed):
    """fp32 [n_r]: random draws; every third candidate sits one ulp below its block's fp32 threshold (hit), the ones after them exactly on it (strict <: no hit)"""
    _, _, n_cand, thrs, _ = lottery_ref(mod, sid, None, 0, mask_prob)
    r = _rng(seed).random(max(n_r, 1), F32N)[:n_r]
    for i in range(min(n_r, n_cand)):
        if i % 3 == 0:
            r[i] = np.nextafter(thrs[i], F32N(-1))
        elif i % 3 == 1:
            r[i] = thrs[i]
    return r


# ------------------------------------------------------------------------------------------------ packed layouts shared by rope and lottery
def _row(L, pieces, tail=(0, -1)):
    """one row from (modality, id, length) pieces, cut at L; the rest is `tail` = (modality, id) padding"""
    m, s, pos = np.full(L, tail[0], np.int64), np.full(L, tail[1], np.int64), 0
    for md, i, n in pieces:
        n = min(n, L - pos)
        m[pos:pos + n], s[pos:pos + n] = md, i
        pos += n
        if pos >= L:
            break
    return m, s


def _cut_row(L, cuts, kind):
    """pieces between the sorted cut points; kind `mod`: modality alternates text / image and the id rises every second piece; `id_txt` / `id_img`: one modality, the id
    rises at every cut (an id change inside a text stretch / inside ONE image run)"""
    cuts = sorted({c for c in cuts if 0 < c < L})
    edges = [0] + cuts + [L]
    pieces = []
    for i in range(len(edges) - 1):
        n = edges[i + 1] - edges[i]
        pieces.append((i % 2, i // 2, n) if kind == "mod" else (0 if kind == "id_txt" else 1, i % 5, n))
    return _row(L, pieces)


def layout_rows(L):
    """the rows of length L, as (name, modality, sample id)"""
    C = (L + 255) // 256
    last = (L + C - 1) // C - 1                                   # the last thread that owns a position
    tids = sorted({t for t in (1, 2, 3, 100, last - 1, last) if 0 < t <= last})
    rows = []
    for d in (-1, 0, 1):
        cuts = [t * C + d for t in tids]
        for kind in ("mod", "id_txt", "id_img"):
            rows.append((f"seam{d:+d}-{kind}", *_cut_row(L, cuts, kind)))
    rows.append(("one-image-run", *_row(L, [(1, 0, L)])))
    rows.append(("image-from-7", *_row(L, [(0, 0, 7), (1, 0, L)])))
    rows.append(("all-text", *_row(L, [(0, 0, L)])))
    rows.append(("all-padding", *_row(L, [])))
    rows.append(("all-padding-mod-1", *_row(L, [], tail=(-1, -1))))
    rows.append(("padding-in-the-middle", *_row(L, [(0, 0, 6), (0, -1, 9), (0, 1, 50), (1, 1, 16), (0, -1, 3), (1, 2, 16), (0, 2, 5)], tail=(-1, -1))))
    pieces = []
    for k, s in enumerate((4, 16, 64)):                           # supported sizes and their neighbours, a text piece of 4 / 5 / 6 tokens between them
        for j, n in enumerate((s, s - 1, s + 1)):
            pieces += [(1, k, n), (0, k, 4 + j)]
    rows.append(("sizes", *_row(L, pieces)))
    rows.append(("sizes-shifted", *_row(L, [(0, 0, 3)] + pieces[::-1])))
    # two image runs of sample 0 separated by a run of sample 1: j counts by id; then blocks of exactly 4 and 5 tokens in one (row, id) - n = 3 and n = 7 candidates
    rows.append(("j-by-id", *_row(L, [(1, 0, 4), (0, 1, 3), (1, 1, 4), (0, 0, 2), (1, 0, 4), (0, 0, 5), (1, 0, 16), (0, 1, 9), (1, 1, 16)])))
    rows.append(("blocks-4-5", *_row(L, [(m, 0, n) for m, n in zip((0, 1) * 3, (5, 4, 5, 4, 5, 4))] + [(m % 2, 1, 5) for m in range(7)] + [(0, 2, 4), (1, 2, 5)])))
    if L == 777:
        rows.append(("alternating-1", *_row(L, [(l % 2 == 0, l // 64, 1) for l in range(L)])))          # 389 run starts: the second round of the j loop
    if L == 1536:
        rows.append(("alternating-5", *_row(L, [(q % 2, q // (3 if q < 150 else 7), 5) for q in range(308)])))   # 307 candidates: second round of the decide loop
    return rows


def layout_cases():
    """cases of at most 5 rows: dict(name, L, mod, sid, rows = the row names)"""
    out = []
    for L in LENGTHS:
        rows = layout_rows(L)
        seen, uniq = set(), []
        for name, m, s in rows:                                   # short rows repeat (every cut is clipped away): keep one of each
            key = (m.tobytes(), s.tobytes())
            if key not in seen:
                seen.add(key)
                uniq.append((name, m, s))
        for c in range(0, len(uniq), 5):
            chunk = uniq[c:c + 5]
            out.append(dict(name=f"L{L}-{c // 5}", L=L, rows=[n for n, _, _ in chunk], mod=np.stack([m for _, m, _ in chunk]), sid=np.stack([s for _, _, s in chunk])))
    return out


def lottery_configs(n_cand):
    """(mask_prob, n_r) of a layout with n_cand candidates: every probability with more uniforms than candidates; one uniform short; none at all (r null)"""
    return [(p, n_cand + 3) for p in MASK_PROBS] + [(0.9, max(n_cand - 1, 0)), (0.9, 0)]


# ------------------------------------------------------------------------------------------------ timestep and noise schedule
def t_noise_consts():
    """the three fp32 arguments of the entry point: fp32(1 - sampling_eps), fp32(sampling_eps), fp32(1 - eps)"""
    return F32N(1 - SEPS), F32N(SEPS), F32N(1 - NEPS)


def t_noise_ieee(u, antithetic, cpu_division=False, mutant=None):
    """(t, dsigma) fp32 [n]: the kernel's operations, one IEEE fp32 rounding each.  cpu_division: u / n and i / n as divisions, what torch does on the
    CPU (on the device, and in the kernel, a division by a host scalar is a product with its fp32 reciprocal); scalar / tensor is reciprocal-then-multiply everywhere"""
    c, eps, c1 = t_noise_consts()
    n = len(u)
    e = np.asarray(u, F32N)
    if antithetic:
        i = (np.arange(n) + (1 if mutant == "offset_i_plus_1" else 0)).astype(F32N)
        if cpu_division:
            e = np.fmod(e / F32N(n) + i / F32N(n), F32N(1))
        else:
            inv_n = F32N(1) / F32N(n)
            e = np.fmod(e * inv_n + i * inv_n, F32N(1))
    t = c * e + eps
    den = F32N(1) - c1 * t
    return t, (F32N(1) / den) * c1


def t_noise_64(t):
    """(sigma64, move64, E_sigma / (FACTOR W), E_move / (FACTOR W)) at the fp32 t"""
    c1 = F64N(t_noise_consts()[2])
    x = c1 * np.asarray(t, F64N)
    sigma = -np.log1p(-x)
    move = -np.expm1(-sigma)
    S_sigma = sigma + x / (1 - x)
    S_move = move + (1 - move) * (1 + sigma) + x
    return sigma, move, U * S_sigma, U * S_move


def t_noise_f32(t):
    """sigma and the move chance in torch CPU fp32 ops, the kernel's order"""
    c1 = float(t_noise_consts()[2])
    tt = torch.from_numpy(np.asarray(t, F32N))
    sg = -torch.log1p(-c1 * tt)
    return sg.numpy(), (1 - torch.exp(-sg)).numpy()


def t_noise_u(n, seed):
    """fp32 [n] in [0, 1): random draws with 0, 1 - 2^-24 (u / n + i / n rounds up to (i + 1) / n - the last sample wraps to 0) and 1 - 2^-23 among them"""
    u = _rng(seed * 31 + n).random(n, F32N)
    u[0] = 0.0
    for k, v in ((1, 1 - 2.0 ** -24), (2, 1 - 2.0 ** -23), (n - 1, 1 - 2.0 ** -24), (n - 2, 0.0)):
        if seed % 2 == 0 and 0 <= k < n:
            u[k] = v
    return u


def t_noise_properties(t, move, antithetic):
    """the properties of the issue, as the number of samples that miss each: t in [eps, 1]; antithetic: sample i in its stratum, widened by 8 u (inv_n, two products
    and a sum on e <= 1, then two more roundings: 5 u, rounded up) - the last sample may wrap into the first stratum, as the reference's % 1 does; move in [0, 1);
    |move - c' t| <= E_move"""
    c, eps, c1 = (F64N(v) for v in t_noise_consts())
    t64, n = np.asarray(t, F64N), len(t)
    out = dict(t_range=int(((t64 < eps) | (t64 > 1)).sum()), move_range=int(((move < 0) | (move >= 1)).sum()))
    if antithetic:
        i = np.arange(n)
        lo, hi = eps + c * i / n - 8 * U, eps + c * (i + 1) / n + 8 * U
        ok = (t64 >= lo) & (t64 <= hi)
        ok[n - 1] |= t64[n - 1] <= eps + c / n + 8 * U
        out["stratum"] = int((~ok).sum())
    E = FACTOR * W_MOVE * t_noise_64(t)[3]
    out["move_is_ct"] = int((np.abs(np.asarray(move, F64N) - c1 * t64) > E).sum())
    return out


# ------------------------------------------------------------------------------------------------ diffusion loss
def sum_chain(N):
    return (N + 1023) // 1024 + 23


def loss_bound(N, case):
    """k of gamma_k for (loss, txt_loss, img_loss, coef) - the module docstring derives them"""
    k = sum_chain(N)
    if case.startswith("mean") or case == "all_padding":
        return dict(loss=k + 1, txt_loss=0, img_loss=0, coef=2)
    if case in ("weighted_cap", "cap_active", "cap_zero"):
        return dict(loss=3 * (k + 4) + 5, txt_loss=3 * (k + 4) + 4, img_loss=k + 4, coef=6 + 2 * (k + 4) + 3)
    return dict(loss=k + 5, txt_loss=k + 4, img_loss=k + 4, coef=6)


def loss_ref(log_p, w_loss, w_std, att, mm, *, weighted, full_mask=False, text_w=1.0, img_w=1.0, ratio=None, mutant=None):
    """(nlls fp32 [B, L] - exact, coef fp64 [B, L], scalars fp64 [8] = loss, txt_loss, img_loss, txt_frac, img_frac, valid_frac, txt_count, img_count).  Terms of
    unattended positions are never looked at (they may be NaN) unless full_mask."""
    B, L = log_p.shape
    wl = np.asarray(w_loss, F64N)[:, None]
    tok = -np.asarray(log_p, F64N) * wl
    nlls = np.where(att, -np.asarray(log_p, F32N) * np.asarray(w_std, F32N)[:, None], F32N(0)).astype(F32N)
    tw, iw = F64N(F32N(text_w)), F64N(F32N(img_w))
    tx = (mm[..., 0] & att) if mm is not None else np.zeros((B, L), bool)
    im = (mm[..., 1] & att) if mm is not None else np.zeros((B, L), bool)
    n_txt, n_img = F64N(tx.sum()), F64N(im.sum())
    sc = np.zeros(8, F64N)
    with np.errstate(all="ignore"):
        txt_frac, img_frac = n_txt / (n_txt + n_img), n_img / (n_txt + n_img)
        sc[3:8] = txt_frac, img_frac, att.sum() / F64N(B * L), n_txt, n_img
        if weighted:
            txt_loss, img_loss = tok[tx].sum() / n_txt * txt_frac * tw, tok[im].sum() / n_img * img_frac * iw
            scale = F64N(1)
            if ratio is not None and not (np.isnan(txt_loss) or np.isnan(img_loss)):
                scale = min(F64N(1), F64N(F32N(ratio)) * img_loss / (txt_loss + F64N(F32N(1e-8))))
            if mutant == "cap_on_image":
                img_loss, s_t, s_i = img_loss * scale, F64N(1), scale
            else:
                txt_loss, s_t, s_i = txt_loss * scale, scale, F64N(1)
            ft, fi = (F64N(1), F64N(1)) if mutant == "coef_without_fraction" else (txt_frac, img_frac)
            c_txt = 0.0 if np.isnan(txt_loss) else ft * tw * s_t / n_txt
            c_img = 0.0 if np.isnan(img_loss) else fi * iw * s_i / n_img
            txt_loss, img_loss = np.nan_to_num(txt_loss, nan=0.0), np.nan_to_num(img_loss, nan=0.0)
            sc[0:3] = txt_loss + img_loss, txt_loss, img_loss
            c = np.where(att, (mm[..., 0] * c_txt + mm[..., 1] * c_img), 0.0)
        else:
            am = np.ones((B, L), bool) if (full_mask or mutant == "mean_counts_unattended") else att
            loss = tok[am].sum() / F64N(am.sum())
            c = np.where(am, 0.0 if np.isnan(loss) else 1.0 / F64N(am.sum()), 0.0)
            sc[0] = np.nan_to_num(loss, nan=0.0)
        coef = -wl * c
    return nlls, coef, sc


def loss_case(B, L, case):
    """inputs of one (shape, case): dict(log_p, w_loss, w_std, att, mm, kw).  The seven cases of tests/test_gpu_kernels.py with their constants; three cap families
    built from the sums so that the fp64 ratio is 0.5 (active), 3 (inactive) or 0 - at least 1e-3 from 1; a token attended but of neither modality."""
    g = _rng(11 * B + L)
    N = B * L
    log_p = (-g.random((B, L)) * 9).astype(F32N)
    sigma, dsigma = g.random(B) * 3 + 0.05, 1 + g.random(B)
    w_std, w_loss = (dsigma / np.expm1(sigma)).astype(F32N), (dsigma / (np.expm1(sigma) + 0.2)).astype(F32N)
    att = g.random((B, L)) < 0.9
    att.reshape(-1)[[0, N - 1]] = True
    is_img = np.zeros((B, L), bool)
    is_img.reshape(-1)[N * 9 // 25:] = True
    if N > 1:
        is_img.reshape(-1)[0] = False
    kw = dict(weighted=case.startswith(("weighted", "cap", "neither")), text_w=0.7, img_w=1.3)
    if case == "weighted_cap":
        kw["ratio"] = 0.25
    if case == "weighted_no_image":
        is_img[:] = False
    if case == "mean_full_mask":
        kw["full_mask"] = True
    if case == "all_padding":
        att[:] = False
        kw["weighted"] = False
    mm = None if case == "mean_no_modality" else np.stack([~is_img, is_img], -1)
    if case == "neither_modality" and N > 2:
        mm.reshape(-1, 2)[1] = False
        mm.reshape(-1, 2)[N // 2] = False
        att.reshape(-1)[[1, N // 2]] = True
    if case.startswith("cap_"):
        _, _, sc = loss_ref(log_p, w_loss, w_std, att, mm, weighted=True, text_w=0.7, img_w=1.3)
        target = dict(cap_active=0.5, cap_inactive=3.0, cap_zero=0.0)[case]
        kw["ratio"] = f32(target * (sc[1] + 1e-8) / sc[2]) if sc[2] > 0 and target else (0.0 if not target else 0.5)
    return dict(log_p=log_p, w_loss=w_loss, w_std=w_std, att=att, mm=mm, kw=kw)


def cap_ratio(c):
    """the fp64 value the min compares with 1 (None without a cap or with an empty modality)"""
    if c["kw"].get("ratio") is None:
        return None
    _, _, sc = loss_ref(c["log_p"], c["w_loss"], c["w_std"], c["att"], c["mm"], **{**c["kw"], "ratio": None})
    return None if sc[2] == 0 or sc[1] == 0 else float(F64N(F32N(c["kw"]["ratio"])) * sc[2] / (sc[1] + F64N(F32N(1e-8))))


def loss_kernel_f32(log_p, w_loss, w_std, att, mm, *, weighted, full_mask=False, text_w=1.0, img_w=1.0, ratio=None):
    """fp32 restatement of the kernel's summation order in numpy (no FMA): thread i % 1024 adds its terms serially, 6 xor-shuffle levels per wave of 64, then the 16
    wave sums serially; the scalar expressions as in csrc/ce.hip.  (coef, scalars) fp32 - the CPU test holds it to loss_ref inside loss_bound."""
    B, L = log_p.shape
    N = B * L
    lp, at = log_p.reshape(-1), att.reshape(-1)
    tok = (-lp * np.repeat(np.asarray(w_loss, F32N), L)).astype(F32N)
    m2 = mm.reshape(-1, 2) if mm is not None else np.zeros((N, 2), bool)

    def block_sum(sel):
        v = np.zeros(((N + 1023) // 1024) * 1024, F32N)
        v[:N] = np.where(sel, tok, F32N(0))
        acc = np.zeros(1024, F32N)
        for row in v.reshape(-1, 1024):
            acc = acc + row
        w = acc.reshape(16, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lane ^ o]
        s = F32N(0)
        for k in range(16):
            s = F32N(s + w[k, 0])
        return s

    tx, im, am = m2[:, 0] & at, m2[:, 1] & at, (np.ones(N, bool) if full_mask else at)
    n_txt, n_img, n_all = F32N(tx.sum()), F32N(im.sum()), F32N(am.sum())
    s_txt, s_img, s_all = block_sum(tx), block_sum(im), block_sum(am)
    with np.errstate(all="ignore"):
        total = F32N(n_txt + n_img)
        txt_frac, img_frac = n_txt / total, n_img / total
        c_txt = c_img = c_all = F32N(0)
        txt_loss = img_loss = F32N(0)
        if weighted:
            txt_loss, img_loss = ((s_txt / n_txt) * txt_frac) * F32N(text_w), ((s_img / n_img) * img_frac) * F32N(img_w)
            scale = F32N(1)
            if ratio is not None and not (np.isnan(txt_loss) or np.isnan(img_loss)):
                scale = min(F32N(1), (F32N(ratio) * img_loss) / (txt_loss + F32N(1e-8)))
            txt_loss = txt_loss * scale
            c_txt = F32N(0) if np.isnan(txt_loss) else (txt_frac * F32N(text_w) * scale) / n_txt
            c_img = F32N(0) if np.isnan(img_loss) else (img_frac * F32N(img_w)) / n_img
            txt_loss, img_loss = F32N(np.nan_to_num(txt_loss)), F32N(np.nan_to_num(img_loss))
            loss = txt_loss + img_loss
            c = np.where(at, np.where(m2[:, 0], c_txt, F32N(0)) + np.where(m2[:, 1], c_img, F32N(0)), F32N(0))
        else:
            loss = s_all / n_all
            c_all = F32N(0) if np.isnan(loss) else F32N(1) / n_all
            loss = F32N(np.nan_to_num(loss))
            c = np.where(am, c_all, F32N(0))
        coef = (-np.repeat(np.asarray(w_loss, F32N), L) * c.astype(F32N)).reshape(B, L)
        sc = np.array([loss, txt_loss, img_loss, txt_frac, img_frac, F32N(at.sum()) / F32N(N), n_txt, n_img], F32N)
    return coef, sc


def loss_judge(N, case, nlls, coef, sc, ref):
    """(mismatches of nlls + counts, worst achieved / bound of {loss, txt_loss, img_loss, frac, coef}) of one output against loss_ref's"""
    n_ref, c_ref, s_ref = ref
    k = loss_bound(N, case)
    bad = same(nlls, n_ref) + same(np.asarray(sc, F64N)[6:8], s_ref[6:8])
    q = dict(frac=ratio(np.asarray(sc)[3:6], s_ref[3:6], U * np.abs(s_ref[3:6])), coef=ratio(coef, c_ref, gamma(k["coef"]) * np.abs(c_ref)))
    for i, name in enumerate(("loss", "txt_loss", "img_loss")):
        q[name] = ratio(np.asarray(sc)[i], s_ref[i], gamma(k[name]) * abs(s_ref[i]) if k[name] else 0.0)
    return bad, q
