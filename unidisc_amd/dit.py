"""MI355X-native drop-in for the reference's ``models/dit.py::DIT``.

Same constructor signature, ``forward`` signature and ``state_dict`` schema as the reference
(models/dit.py:1095-1500), so ``config.backbone == "dit"`` can select this class in
``model_setup.init`` (model_setup.py:134-161) and HF checkpoints load unchanged.  The sub-modules below
exist to own parameters under the reference's names; compute does not go through ``nn.Module.forward``
of the children.  Instead ``DIT`` runs a hand-scheduled engine: every op of the block is a HIP kernel
from ``libunidisc_hip.so`` enqueued on the current stream, activations needed by the backward are
kept in HBM (288 GB: no recompute needed at the BASELINE shapes), and the backward is an explicit
reverse schedule that hands finished gradient ranges to an optional callback (used by
``unidisc_amd.ddp`` to overlap the bf16 gradient all-reduce with the rest of the backward).

Numerics follow the reference's bf16-autocast flow: fp32 residual stream and master
weights, bf16 GEMM operands with fp32 accumulation, bf16 activations between GEMMs, fp32 statistics.
Only bf16 compute is implemented (``trainer.precision=bf16``, the reference's training precision).
"""
from __future__ import annotations

import math
import types
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import weakref

import torch
import torch.nn as nn

from . import kernels as K
from .rope import lumina_rope_2d, rotary_table_1d

try:  # optional, for from_pretrained / push_to_hub parity with the reference class
    from huggingface_hub import PyTorchModelHubMixin as _HubMixin
except Exception:  # pragma: no cover
    class _HubMixin:  # type: ignore
        pass

BF16, F32 = torch.bfloat16, torch.float32


def cfg_get(node, key, default=None):
    """getattr/getitem with default over OmegaConf nodes, attribute bags and dicts (the reference leans on getattr(cfg, k, default))."""
    if node is None:
        return default
    if isinstance(node, dict):
        return node.get(key, default)
    try:
        v = getattr(node, key)
    except (AttributeError, KeyError):
        return default
    return v


def static_modality(B, L, static_img_sl, device):
    """The modality map [B, L] of the static layout, written out: 1 (image) inside `static_img_sl`, 0 (text) elsewhere."""
    mod = torch.zeros((B, L), dtype=torch.int64, device=device)
    mod[:, static_img_sl] = 1
    return mod


def _ceil(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------
# parameter containers (names == reference state_dict keys)
# ------------------------------------------------------------------------------------------------
class EmbeddingLayer(nn.Module):  # models/dit.py:1036-1043
    def __init__(self, dim, vocab_dim):
        super().__init__()
        self.embedding = nn.Parameter(torch.empty((vocab_dim, dim)))
        torch.nn.init.kaiming_uniform_(self.embedding, a=math.sqrt(5))


class RMSNorm(nn.Module):  # models/dit.py:77-100
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))


class LayerNorm(nn.Module):  # models/dit.py:383-403 (weight only)
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones([dim]))
        self.dim = dim


def get_norm(dim, norm_type="layernorm"):
    if norm_type == "layernorm":
        return LayerNorm(dim)
    if norm_type == "rms":
        return RMSNorm(dim)
    raise ValueError(f"Unknown norm type: {norm_type}")


class TimestepEmbedder(nn.Module):  # models/dit.py:415-449
    def __init__(self, hidden_size, frequency_embedding_size=256):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(frequency_embedding_size, hidden_size, bias=True), nn.SiLU(), nn.Linear(hidden_size, hidden_size, bias=True))
        self.frequency_embedding_size = frequency_embedding_size


class Attention(nn.Module):  # models/dit.py:515-575
    def __init__(self, dim, n_heads, qk_norm=False):
        super().__init__()
        self.n_heads, self.head_dim, self.qk_norm = n_heads, dim // n_heads, qk_norm
        self.attn_qkv = nn.Linear(dim, 3 * dim, bias=False)
        self.attn_out = nn.Linear(dim, dim, bias=False)
        if qk_norm:
            self.q_norm = nn.LayerNorm(dim)
            self.k_norm = nn.LayerNorm(dim)


class DDiTBlock(nn.Module):  # models/dit.py:890-934
    def __init__(self, dim, n_heads, cond_dim, mlp_ratio=4, dropout=0.1, time_conditioning=True, norm_type="layernorm", sandwich_normalization=False,
                 qk_norm=False):
        super().__init__()
        self.time_conditioning, self.dropout, self.sandwich_normalization = time_conditioning, dropout, sandwich_normalization
        self.attention = Attention(dim, n_heads, qk_norm=qk_norm)
        self.norm1 = get_norm(dim, norm_type)
        self.norm2 = get_norm(dim, norm_type)
        self.mlp = nn.Sequential(nn.Linear(dim, mlp_ratio * dim, bias=True), nn.GELU(approximate="tanh"), nn.Linear(mlp_ratio * dim, dim, bias=True))
        if time_conditioning:
            self.adaLN_modulation = nn.Linear(cond_dim, 6 * dim, bias=True)
            self.adaLN_modulation.weight.data.zero_()
            self.adaLN_modulation.bias.data.zero_()
        if sandwich_normalization:
            self.post_ff_norm = get_norm(dim, norm_type)
            self.pre_residual_norm = get_norm(dim, norm_type)


class DDitFinalLayer(nn.Module):  # models/dit.py:1063-1092
    def __init__(self, hidden_size, out_channels, cond_dim, time_conditioning=True, norm_type="layernorm", zero_linear_init=True):
        super().__init__()
        self.time_conditioning = time_conditioning
        self.norm_final = get_norm(hidden_size, norm_type)
        self.linear = nn.Linear(hidden_size, out_channels)
        if zero_linear_init:
            self.linear.weight.data.zero_()
        self.linear.bias.data.zero_()
        if time_conditioning:
            self.adaLN_modulation = nn.Linear(cond_dim, 2 * hidden_size, bias=True)
            self.adaLN_modulation.weight.data.zero_()
            self.adaLN_modulation.bias.data.zero_()


class ModalityMask:
    """What the reference's `get_block_mask(txt_batch_attn_dropout, img_batch_attn_dropout, txt_length, ...)` (model_utils.py:721-737) describes: in
    samples with txt_drop[b] text queries attend to text keys only, with img_drop[b] image queries to image keys only (positions < txt_length are
    text).  Passed as `block_mask=` where the reference passes its FlexAttention BlockMask."""

    def __init__(self, txt_drop, img_drop, txt_length):
        self.txt_drop, self.img_drop, self.txt_length = txt_drop.reshape(-1).bool(), img_drop.reshape(-1).bool(), int(txt_length)


def ar_head_operands(x0, modality, mask_index):
    """The AR baseline's shifted head (model.py:717-781, :935-967 with trainer.ar_shift) as operands of the fused SUBS cross-entropy, per flat row:
      - "xt": mask_index on every row that has a target - the SUBS log-prob of a [MASK] row IS the AR log-prob (log-softmax with the [MASK] column, and
        under restrict_modality the other modality's ids, excluded) - and a non-mask id on the last position of each sequence, which has no target: its
        log p is 0 with a zero gradient, and the compacted head leaves it out like any unmasked row;
      - the target x0[:, r + 1] (on the last position: that same non-mask id, so that its one-hot log-prob is exactly 0);
      - the TARGET's modality, modality[:, r + 1] (model.py:760-765 `(modality == k)[..., 1:]`): the per-modality head splits its rows by it, so the row
        in front of the first image token (row txt_len - 1) goes to the image head.
    x0, modality: int [B, L] (modality may be None).  Returns three flat int64 tensors [B L] (the third None without modality)."""
    B, L = x0.shape
    x0 = x0.to(torch.int64)
    none = 1 if mask_index == 0 else 0
    ce_ids = torch.full((B, L), mask_index, dtype=torch.int64, device=x0.device)
    ce_ids[:, -1] = none
    tgt = torch.cat([x0[:, 1:], torch.full((B, 1), none, dtype=torch.int64, device=x0.device)], 1)
    mod = None
    if modality is not None:
        modality = modality.to(torch.int64)
        mod = torch.cat([modality[:, 1:], modality[:, -1:]], 1).contiguous().view(-1)
    return ce_ids.view(-1), tgt.contiguous().view(-1), mod


class _Lin:
    """bf16 shadows of one nn.Linear weight: w16 [out(p), in] for forward, w16t [in, out(p)] for dgrad."""

    def __init__(self, weight: nn.Parameter, bias: Optional[nn.Parameter], out_pad: int = 8):
        self.weight, self.bias = weight, bias
        self.out, self.inp = weight.shape
        self.outp = _ceil(self.out, out_pad)
        self.w16 = self.w16t = None
        self.sticky_t = False
        self.need_t = True   # False: every dgrad of this layer reads W itself (K.gemm_nn), the per-step cast writes no transposed shadow

    def alloc(self):
        dev = self.weight.device
        if self.w16 is None or self.w16.device != dev:
            self.w16 = torch.zeros((self.outp, self.inp), dtype=BF16, device=dev)
            self.w16t = None
        if self.need_t and self.w16t is None:
            self.w16t = torch.zeros((self.inp, self.outp), dtype=BF16, device=dev)
        if not self.need_t:
            self.w16t = None

    def refresh(self):
        self.alloc()
        K.cast_transpose(self.weight.detach(), self.w16, self.w16t)

    def dgrad_form(self):
        """Which operand the dgrad of a forward that runs NOW will read, decided at FORWARD time and carried to the backward in the forward's saved state:
        "nt" = the transposed shadow (it exists for this forward and, being sticky, for every later one), "nn" = W's forward shadow (no transposed one is kept)."""
        return "nt" if self.w16t is not None else "nn"

    def dgrad(self, dY, M_rows, form=None):
        """dX [M, in] = dY [M, out] W in the form the forward recorded (`dgrad_form`); a transposed shadow that appeared since (another forward with a row
        count outside gemm_nn made it sticky) is current and takes over an "nn" record whose shape no longer fits - never the other way round."""
        form = self.dgrad_form() if form is None else form
        if form == "nt" or (self.w16t is not None and not K.gemm_nn_ok(M_rows, self.inp, self.out)):
            if self.w16t is None:
                raise RuntimeError(f"unidisc_amd: the forward of this {self.out}x{self.inp} Linear recorded an NT dgrad but its transposed weight shadow is gone")
            return K.gemm_nt(dY, self.w16t, N=self.inp)
        if not K.gemm_nn_ok(M_rows, self.inp, self.out):
            raise RuntimeError(f"unidisc_amd: dgrad of a {self.out}x{self.inp} Linear over {M_rows} rows has no transposed weight shadow and the shape is outside gemm_nn")
        return K.gemm_nn(dY, self.w16, N=self.inp)


# ------------------------------------------------------------------------------------------------
# the engine's records
# ------------------------------------------------------------------------------------------------
@dataclass
class _KVRead:
    """Attend to a K / V cache: K, V per block [B, Lmax, d]; slot0: where this call's rows go; Lk: the slots the queries see; split: the conditioning cache's
    form (small batches, the keys split over workgroups where the plan says so) with its workspace `ws`; causal: the chunked cached forward of a causal
    backbone (query i sees the slots j <= i + Lk - L: with slot0 = Lk - L its own slot and everything before it; udm_attention_fwd_kv_causal, no split form)."""
    K: list
    V: list
    slot0: int
    Lk: int
    split: bool = False
    ws: Optional[torch.Tensor] = None
    causal: bool = False


@dataclass
class _EngineInputs:
    """What one engine forward runs on.  Every caller builds this record; what a caller does not say is off."""
    indices: torch.Tensor
    sigma: Optional[torch.Tensor] = None
    modality: Optional[torch.Tensor] = None
    sample_ids: Optional[torch.Tensor] = None
    x0: Optional[torch.Tensor] = None               # "logp": the clean tokens
    restrict: bool = False                          # "logp": restrict_modality
    save: bool = False                              # keep what the backward reads (grad mode is off inside Function.forward, so the caller decides)
    block_mask: object = None                       # a ModalityMask (anything else is ignored)
    key_mask: Optional[torch.Tensor] = None         # the key-padding mask of model.use_attention_mask
    plan_ids: Optional[torch.Tensor] = None         # take the [MASK] row selection from this tensor instead of `indices`
    ar_shift: bool = False                          # "logp": the AR baseline's shifted head
    rope: Optional[tuple] = None                    # (cos, sin) rows of the full-length tables (the cached paths)
    kv_sink: Optional[list] = None                  # per block (K, V): every position's post-rope k and its v go there
    kv_read: Optional[_KVRead] = None
    head_out: Optional[torch.Tensor] = None         # "logits": the head on each row's last position only, into this buffer (KV-cache prefill)


class _Record:
    """Named fields only - a misspelt one is an AttributeError, not a silent None - and every field None until it is set."""
    __slots__ = ()

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __getattr__(self, name):   # (reached only by a name that has no value yet: None for a field, an error for anything else)
        if name not in self.__slots__:
            raise AttributeError(f"{type(self).__name__} has no field {name!r}")


class _Saved(_Record):
    """One forward's context, and with `save` what its backward reads.  It holds tensors and plain values only - nothing callable, nothing that refers back to
    it - so dropping the record frees everything at once."""
    __slots__ = ("mode", "save", "ckpt", "B", "L", "nt", "ids", "modality", "emb_mod", "sid", "doc_ranges", "p_drop", "p_attn", "seed0", "dgrad_form", "cos", "sin",
                 "cnt_j", "kv_sink", "kv_read", "head_plan", "ada_cache", "blocks",                    # the forward's context (what _block_forward reads)
                 "Bp", "te", "l1", "s1", "l2", "c", "any_img",                                        # the sigma map
                 "x_final", "hf", "rstdf", "meanf", "fmod", "logits", "head_rows", "ids_h", "x0", "ce_mod", "restrict", "lse_ce", "stream_compact", "head_chunk",
                 "head_groups")                                                                        # the final layer and the head

    def attn_drop_kw(self, i):
        """Attention-probability dropout of block i: seed slot 4 i + 3 (4 i + 1, 4 i + 2 are the block's residual dropouts).  Passed only when p > 0, like
        _attn_mask_kw.  The forward, the backward and the checkpointing recompute read this one method, so the three kernels of one attention regenerate one mask."""
        return dict(dropout_p=self.p_attn, seed=self.seed0 + 4 * i + 3) if self.p_attn > 0.0 else {}


class _BlockActs(_Record):
    """What one block's backward reads.  Under activation checkpointing (`ckpt`) only the block's input `x_in` and the compacted row list `rows_c`."""
    __slots__ = ("ckpt", "x_in", "rows_c", "mod", "h1", "rstd1", "mean1", "qkv", "qkr", "qstats", "o", "lse", "a_out", "rstd_a", "mean_a", "x_mid", "h2", "rstd2",
                 "mean2", "u1", "g", "u2", "rstd_m", "mean_m", "o_c")


class _PendingNorm(_Record):
    """Without adaLN every pre-norm backward is immediately followed by the backward of the residual branch that produced the norm's input, on the dx it has just
    updated: the pair runs as ONE fused pass (K.norm_residual_bwd; adaLN-Zero, round 5: its modulated / gated form K.norm_residual_bwd_ada where that kernel covers
    the shape).  This record carries the norm half to the branch that consumes it: the norm's operands, with adaLN its modulation `mod` and the chunks `mod_idx` =
    (shift, scale) whose gradients go into `dmod`, and `finish`: the block (n_blocks: the final layer) whose gradient range is reported, and whose activations
    are dropped, only after that pass - the final norm and each block's norm1 pair with the MLP branch of the block below them in the schedule."""
    __slots__ = ("dy", "x", "rstd", "mean", "w", "dw", "accumulate", "mod", "dmod", "mod_idx", "finish")


class _Backward(_Record):
    """The state of one backward pass: the flat gradient buffer and its per-parameter views G, the residual-stream gradient dx, the pending norm, and with adaLN
    dc and the partial tiles the adaLN_modulation backwards leave for `_sigma_map_backward` (`ada_buf`, filled up to `ada_off`)."""
    __slots__ = ("S", "nt", "flat", "G", "dx", "dc", "pend", "tc_fused", "ada_buf", "ada_off")


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
class _DecodeGraph:
    """One captured decode step of a DIT on its KV cache (DIT.capture_decode_step).  Holds the addresses of the cache's buffers: it is valid until the
    next reset_kv_cache and must be dropped before it."""

    def __init__(self, dit, tail):
        kv = dit._kv
        self._dit, self._kv = weakref.ref(dit), kv

        def step():
            dit._decode_step_at()
            if tail is not None:
                tail()
            K.counter_add(kv.pos_dev, 1)

        ids0, pos0 = kv.ids.clone(), kv.pos_dev.clone()
        step()                                   # warm-up, undone below
        kv.ids.copy_(ids0), kv.pos_dev.copy_(pos0)
        torch.cuda.current_stream().synchronize()
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph):
                step()
        except Exception as e:   # (a launch refused under capture answers through udm_last_error: the message names it)
            self.graph = None
            raise RuntimeError(f"unidisc_amd.DIT.capture_decode_step: the runtime rejected the capture of the decode step: {e}") from e

    def replay(self):
        """one graph launch: the decode step at the device's position, the token choice, position + 1"""
        dit = self._dit()
        if dit is None or dit._kv is not self._kv or self.graph is None:
            raise RuntimeError("unidisc_amd.DIT: this captured decode step belongs to a KV cache that was reset")
        self.graph.replay()
        self._kv.pos += 1


class DIT(nn.Module, _HubMixin):
    def __init__(self, config, vocab_size: int, text_vocab_size: int, mask_index: int, dtype=None, device=None, static_img_sl=None, static_txt_sl=None,
                 **kwargs):
        super().__init__()
        self.config = config
        m, tr, data = cfg_get(config, "model"), cfg_get(config, "trainer"), cfg_get(config, "data")
        self.autocast_dtype = dtype
        self.vocab_size, self.text_vocab_size, self.mask_index = vocab_size, text_vocab_size, mask_index
        self.time_conditioning = bool(cfg_get(config, "time_conditioning", False) or cfg_get(m, "force_time_conditioning", False))
        # trainer.use_gradient_checkpointing (models/dit.py:1486-1490: every block is recomputed in the backward; the reference needs it on 48 GB parts): the
        # engine then keeps only each block's input (and the head's activations) and re-runs the block's forward right before its backward - same kernels,
        # same dropout seeds, bit-identical gradients (tests/test_engine_orchestration.py, tests/test_gpu_e2e.py).  Off, a block's activations stay resident
        # (0.92 GB per block at 1.4 B, B = 8: 22 GB of 288 GB), which is the faster choice whenever they fit.
        self.use_gradient_checkpointing = bool(cfg_get(tr, "use_gradient_checkpointing", False))
        self.sandwich_normalization = cfg_get(m, "sandwich_normalization", False)
        self.static_img_sl, self.static_txt_sl = static_img_sl, static_txt_sl
        for flag, why in (("img_cond", "cross-attention image conditioning"), ("cond_label", "class-label conditioning"),
                          ("use_pretrained_img_emb", "pretrained VQ embedding table"), ("use_flex_attention_cache", "inference modality KV cache")):
            if cfg_get(m, flag, False):
                raise NotImplementedError(f"unidisc_amd.DIT: model.{flag} ({why}) is outside the denoising hot path (SURVEY.md §8)")
        # model.use_kv_cache (models/dit.py:588-607, 776-780, 1462-1473): the AR sampler's per-block K / V cache and its one-token decode step
        # (reset_kv_cache / forward(start_pos=...)) - a causal cache, so only for causal backbones
        self.use_kv_cache = bool(cfg_get(m, "use_kv_cache", False))
        if self.use_kv_cache and cfg_get(m, "full_attention", True):
            raise NotImplementedError("unidisc_amd.DIT: model.use_kv_cache (inference KV cache) needs a causal backbone (model.full_attention=false, the AR "
                                      "baseline): a bidirectional block's keys change with every new token")
        self._kv = self._mc = self._cc = None
        # model.full_attention=false (models/dit.py:1118, the AR baseline of configs/experiments/ar.yaml): every block attends causally (sdpa is_causal=True,
        # :768 / :826 / :843) - the attention kernels' UDM_ATTN_CAUSAL form.  The reference never combines it with another mask: an attention_mask beside
        # is_causal is an SDPA error, and the packed / flex-mask paths sit inside `parameterization != "ar"`.
        self.causal = not cfg_get(m, "full_attention", True)
        self._attn_mask_kw = dict(causal=True) if self.causal else {}   # (bidirectional blocks call the attention entry points exactly as before)
        if self.causal:
            if cfg_get(data, "require_sample_ids", False):
                raise NotImplementedError("unidisc_amd.DIT: causal attention (model.full_attention=false) with data.require_sample_ids (packed documents) - "
                                          "the reference has no causal document mask")
            if cfg_get(m, "use_attention_mask", False):
                raise NotImplementedError("unidisc_amd.DIT: causal attention (model.full_attention=false) with model.use_attention_mask - an attention mask "
                                          "beside is_causal is an SDPA error in the reference")
        if cfg_get(tr, "image_mode", "discrete") == "continuous":
            raise NotImplementedError("unidisc_amd.DIT: continuous image mode is not on the denoising hot path")
        # model.attn_dropout (configs/experiments/jan_cub.yaml; models/dit.py:1179, :1265 -> sdpa(dropout_p=attn_dropout if training else 0), :825-829, on the
        # bidirectional and on the causal path): dropout on the softmax probabilities, inside the attention kernels.  The reference's FlexAttention path
        # (:784-812: packed documents, modality masking) draws none; the key-padding mask shares the kernels' id slot with those and is left out with them.
        self.attn_dropout = float(cfg_get(m, "attn_dropout", None) or 0.0)
        if self.attn_dropout > 0.0:
            if not self.attn_dropout < 1.0:
                raise ValueError(f"unidisc_amd.DIT: model.attn_dropout = {self.attn_dropout} must be in [0, 1)")
            if cfg_get(data, "require_sample_ids", False):
                raise NotImplementedError("unidisc_amd.DIT: model.attn_dropout with data.require_sample_ids (packed documents) - the reference's FlexAttention "
                                          "path applies no attention dropout")
            if cfg_get(m, "flex_attention_txt_masking_prob", None) is not None or cfg_get(m, "flex_attention_img_masking_prob", None) is not None:
                raise NotImplementedError("unidisc_amd.DIT: model.attn_dropout with model.flex_attention_{txt,img}_masking_prob (modality masking) - the "
                                          "reference's FlexAttention path applies no attention dropout")
            if cfg_get(m, "use_attention_mask", False):
                raise NotImplementedError("unidisc_amd.DIT: model.attn_dropout with model.use_attention_mask - the dropout kernels take no key-padding mask")

        d, H = cfg_get(m, "hidden_size"), cfg_get(m, "n_heads")
        self.hidden_size, self.n_heads, self.head_dim = d, H, d // H
        self.cond_dim, self.n_blocks = cfg_get(m, "cond_dim"), cfg_get(m, "n_blocks")
        self.norm_type, self.qk_norm = cfg_get(m, "norm_type", "layernorm"), cfg_get(m, "qk_norm", False)
        self.dropout = float(cfg_get(m, "dropout", 0.0) or 0.0)
        if self.head_dim not in (32, 64, 128, 256):
            raise NotImplementedError(f"unidisc_amd.DIT: head_dim {self.head_dim} unsupported (32/64/128/256)")

        self.vocab_embed = EmbeddingLayer(d, vocab_size)
        self.sigma_map = TimestepEmbedder(self.cond_dim) if self.time_conditioning else None
        self.modality_embed = EmbeddingLayer(d, 2) if cfg_get(m, "modality_embed", False) else None

        self.txt_length, self.img_length, self.total_length = cfg_get(m, "txt_length"), cfg_get(m, "img_length"), cfg_get(m, "length")
        self.multimodal_batches = bool(cfg_get(tr, "multimodal_batches", False))
        self.rope_2d = bool(cfg_get(m, "rope_2d", False))
        # The softmax scale lives in the stored q: the qk-norm + rope kernel writes bf16(q log2(e) / sqrt(D)) - one rounding, where the reference rounds q and
        # flash-attn scales the fp32 scores - so the attention kernels' scores are base-2 exponents as they leave the matrix pipe (no multiply per score in
        # the forward or in either backward kernel); the rope backward multiplies the incoming dq by the same factor.
        self.attn_q_scale = K.attention_q_scale(self.head_dim)
        # model.head_chunk_rows (extension key, 0 = off): fused vocabulary head + SUBS cross-entropy that never materialises [rows, V] logits - the head
        # runs on chunks of this many rows (forward: logits chunk -> log p, dropped; backward: the chunk's logits are recomputed, d logits formed in
        # place and consumed by the dgrad / wgrad).  Trades one extra head GEMM per step for rows * V * 2 bytes of peak memory (SURVEY K11 + K12).
        self.head_chunk_rows = int(cfg_get(m, "head_chunk_rows", 0) or 0)
        self.require_sample_ids = bool(cfg_get(data, "require_sample_ids", False))
        assert (self.txt_length + self.img_length == self.total_length) or self.multimodal_batches
        self._register_rotary_tables(cfg_get(m, "linear_factor", 1.0))

        self.blocks = nn.ModuleList([
            DDiTBlock(d, H, self.cond_dim, dropout=self.dropout, time_conditioning=self.time_conditioning, norm_type=self.norm_type,
                      sandwich_normalization=self.sandwich_normalization, qk_norm=self.qk_norm) for _ in range(self.n_blocks)
        ])
        self.output_layer = DDitFinalLayer(d, vocab_size, self.cond_dim, time_conditioning=self.time_conditioning, norm_type=self.norm_type,
                                           zero_linear_init=cfg_get(m, "zero_linear_init", True))
        self.allow_compiled_embed = False
        if device is not None:
            self.to(device)
        # engine state
        self._lins: Optional[Dict[str, _Lin]] = None
        self._fwd_count = 0
        self.compact_head = True          # "logp" mode: run the vocabulary head on the [MASK] rows only (exact: other rows have log p = 0)
        # ... and with it everything of the LAST block behind its attention (out-proj, residual adds, MLP, final norm): only the head reads that
        # block's output, so its unmasked rows feed nothing and receive a zero gradient (exact; no adaLN: the row kernels would need the row -> sample map)
        self.compact_last_block = os.environ.get("UDM_COMPACT_LAST", "1") != "0"
        # SUBS with force_argmax_valid_indices: a text row's logits matter on the text ids only, an image row's on the image ids only (everything else is -inf in the
        # forward and has a zero gradient) - the head (forward, dgrad, wgrad) then runs as (text rows x text ids) + (image rows x image ids) instead of rows x all ids
        self.split_head = os.environ.get("UDM_SPLIT_HEAD", "1") != "0"
        self.pair_wgrads = os.environ.get("UDM_PAIR_WGRADS", "1") != "0"   # qkv + out-proj weight gradients in one 256-tile launch (K.gemm_tn_pair)
        # the four weight gradients of a block in ONE split-K launch + ONE reduce where each of them is a few tiles over the long row contraction (UniDisc-S)
        self.multi_wgrads = os.environ.get("UDM_MULTI_WGRADS", "1") != "0"
        self.dgrad_from_w = os.environ.get("UDM_DGRAD_NN", "1") != "0"   # dgrads from the forward's W shadow where the shape allows (see refresh_weight_shadows)
        self.grad_ready_callback = None   # fn(flat_grads, lo, hi): elements [lo, hi) of this backward's flat fp32 gradient buffer are final
        self.grad_sync_finish = None      # fn(): called at the end of backward (e.g. make the compute stream wait for the all-reduces)
        self.recast_every_forward = True  # mirror autocast: fp32 master -> bf16 shadow on every training forward
        self.overlap_weight_cast = os.environ.get("UDM_OVERLAP_CAST", "0") != "0"   # opt-in: the casts on a side stream under the blocks before (measured: no gain, 96.1 vs 96.2 ms)
        self._shadow_versions = None

    def _register_rotary_tables(self, linear_factor):
        D = self.head_dim
        if self.rope_2d:  # models/dit.py:1203-1232
            if not (self.multimodal_batches and self.modality_embed is not None):
                raise NotImplementedError("unidisc_amd.DIT: rope_2d needs multimodal_batches and modality_embed (as in every shipped config)")
            if self.require_sample_ids:  # interleaved / packed batches (:1209-1216): one table per supported image block, image-count embedding
                for n_img, lf in self.IMG_BLOCKS:
                    side = int(math.sqrt(n_img))
                    emb = self._lumina(D, side, side, lf)
                    self.register_buffer(f"rotary_cos_emb_img_{n_img}", emb.flatten(0, 1).real.contiguous(), persistent=False)
                    self.register_buffer(f"rotary_sin_emb_img_{n_img}", emb.flatten(0, 1).imag.contiguous(), persistent=False)
                self.img_count_embedding = nn.Parameter(torch.zeros((16, self.hidden_size)))
            else:
                side = int(math.sqrt(self.img_length))
                assert side * side == self.img_length, f"seq_len_2d must be a square number, got {self.img_length}"
                emb = self._lumina(D, side, side, linear_factor)
                self.register_buffer("rotary_cos_emb_img", emb.flatten(0, 1).real.contiguous(), persistent=False)
                self.register_buffer("rotary_sin_emb_img", emb.flatten(0, 1).imag.contiguous(), persistent=False)
            c, s = rotary_table_1d(self.total_length, D)
            self.register_buffer("rotary_cos_emb_txt", c, persistent=False)
            self.register_buffer("rotary_sin_emb_txt", s, persistent=False)
        else:  # :1234-1239
            c, s = rotary_table_1d(self.total_length, D)
            self.register_buffer("rotary_cos_emb", c, persistent=False)
            self.register_buffer("rotary_sin_emb", s, persistent=False)

    @staticmethod
    def _lumina(D, h, w, linear_factor):
        try:
            from diffusers.models.embeddings import get_2d_rotary_pos_embed_lumina as fn  # the reference's source, when installed
            return fn(D, h, w, linear_factor=linear_factor, ntk_factor=1.0)
        except Exception:
            return lumina_rope_2d(D, h, w, linear_factor=linear_factor, ntk_factor=1.0)

    # Reference API surface that callers touch.  `eval.attention_caching` (model_eval.py:2296-2366): the reference allocates a per-layer
    # K / V buffer here and WRITES it in the cache-building / text-only steps (models/dit.py:797-803), but no forward ever reads it back (:812 attends
    # to the keys of the current input only).  The default path reproduces that and needs no state in the backbone: `Diffusion.sample` passes the
    # image-queries-see-image-keys mask / the text slice itself, and the two calls are accepted and remembered for callers that probe them.
    # The read-cache path (extension key eval.attention_caching_read_cache, set_flex_attention_cache(..., read_cache=True)) does what the reference's
    # comment at :790-792 intends and DOES need state: per block bf16 K / V [B, L, d], filled by the build step and read by every text step
    # (forward_masked_logits(modality_cache=...)); reset_kv_cache() frees it.
    #
    # With arguments (`_ar_sampler`, model_eval.py:2736-2822) it is the AR baseline's KV cache: per block bf16 K / V [rows, seq_len, d] (rows padded to a
    # multiple of 8), the decode step's buffers and its rotary rows, allocated once here.  `modality` (extension, full length [batch_size, model.length]):
    # the decode step at position p then takes its modality-embedding ids and - with 2-D rope - its rotary rows from row p of the FULL-length tables
    # (the ones training used), so decode step p equals row p of the causal forward.  set_to_none=True frees everything.
    def reset_kv_cache(self, batch_size=None, seq_len=None, dtype=None, device=None, set_to_none=False, modality=None):
        self.use_flex_attention_cache = False
        self._mc = None   # the modality K / V cache of set_flex_attention_cache(read_cache=True)
        self._cc = None   # the conditioning K / V cache of set_conditioning_cache
        if set_to_none:
            self._kv = None
            return
        if batch_size is None:
            return
        if not self.causal:
            raise NotImplementedError("unidisc_amd.DIT.reset_kv_cache: model.use_kv_cache needs a causal backbone (model.full_attention=false)")
        if self.time_conditioning:
            raise NotImplementedError("unidisc_amd.DIT.reset_kv_cache: the decode step has no adaLN (time_conditioning); the AR baseline has no sigma")
        dev = torch.device(device) if device is not None else self.vocab_embed.embedding.device
        B, Lmax = int(batch_size), int(seq_len)
        Bp = _ceil(B, 8)
        if Bp > K.SKINNY_MAX_ROWS:
            raise NotImplementedError(f"unidisc_amd.DIT.reset_kv_cache: {B} rows (padded {Bp}); the decode step serves at most {K.SKINNY_MAX_ROWS} rows")
        if not 1 <= Lmax <= self.total_length:
            raise ValueError(f"unidisc_amd.DIT.reset_kv_cache: seq_len {Lmax} outside [1, model.length = {self.total_length}]")
        self._kv = None
        self._refresh_shadows_now()
        d, H, D = self.hidden_size, self.n_heads, self.head_dim
        Lt = self.total_length
        kv = types.SimpleNamespace(B=B, Bp=Bp, Lmax=Lmax, pos=0)
        kv.K = [torch.zeros((Bp, Lmax, d), dtype=BF16, device=dev) for _ in self.blocks]
        kv.V = [torch.zeros((Bp, Lmax, d), dtype=BF16, device=dev) for _ in self.blocks]
        kv.ids = torch.zeros(Bp, dtype=torch.int64, device=dev)
        # the step's buffers: residual stream ping-pong (x -> x_mid -> x), one bf16 norm output, row statistics nobody reads back
        kv.x = [torch.empty((Bp, d), dtype=F32, device=dev) for _ in range(2)]
        kv.h = torch.empty((Bp, d), dtype=BF16, device=dev)
        kv.stat = [torch.empty(Bp, dtype=F32, device=dev) for _ in range(4)]
        kv.qkr = torch.empty((Bp, 2 * d), dtype=BF16, device=dev)
        kv.qstats = torch.empty((Bp, 4), dtype=F32, device=dev)
        kv.qkv = torch.empty((Bp, 3 * d), dtype=BF16, device=dev)
        kv.o = torch.empty((Bp, d), dtype=BF16, device=dev)
        kv.a_out = torch.empty((Bp, d), dtype=BF16, device=dev)
        kv.g = torch.empty((Bp, 4 * d), dtype=BF16, device=dev)
        kv.u2 = torch.empty((Bp, d), dtype=BF16, device=dev)
        kv.logits = torch.empty((Bp, self._lins["head"].outp), dtype=BF16, device=dev)
        need = max(K.skinny_ws_elems(Bp, N, Kd) for N, Kd in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d), (self.vocab_size, d)))
        kv.gws = torch.empty(max(need, 4), dtype=F32, device=dev)   # the K splits of the step's five GEMM shapes
        kv.aws = K.attention_decode_ws(Bp, H, D, dev)
        mod_full = None
        if modality is not None:
            modality = modality.to(dev).to(torch.int64)
            if tuple(modality.shape) != (B, Lt):
                raise ValueError(f"unidisc_amd.DIT.reset_kv_cache: modality must be the full-length map [{B}, {Lt}], got {tuple(modality.shape)}")
            mod_full = torch.cat([modality, modality[:1].expand(Bp - B, Lt)], 0) if Bp > B else modality
        elif self.modality_embed is not None or self.rope_2d:
            if self.multimodal_batches:
                raise ValueError("unidisc_amd.DIT.reset_kv_cache: modality_embed / rope_2d with multimodal_batches need the full-length `modality`")
            mod_full = self._static_modality(Bp, Lt, dev)
        kv.mod_full = mod_full
        kv.mod_cols = mod_full.t().contiguous() if mod_full is not None else None     # [L, Bp]: the embedding's modality ids of position p, contiguous
        if self.rope_2d:
            cos, sin = self._rotary(mod_full, Lt)                                        # [Bp, L, D/2], the training tables
            kv.cos, kv.sin = cos.transpose(0, 1).contiguous(), sin.transpose(0, 1).contiguous()
        else:
            kv.cos = kv.sin = None
        # the device-side position of _decode_step_at and the fixed one-row operands udm_decode_stage fills from it (what a captured step reads)
        kv.pos_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        kv.mod_row = torch.zeros(Bp, dtype=torch.int64, device=dev) if (kv.mod_cols is not None and self.modality_embed is not None) else None
        kv.rope_tabs = (kv.cos, kv.sin) if kv.cos is not None else (self.rotary_cos_emb.contiguous(), self.rotary_sin_emb.contiguous())
        kv.cos_row, kv.sin_row = torch.zeros_like(kv.rope_tabs[0][:1]), torch.zeros_like(kv.rope_tabs[1][:1])
        self._kv = kv

    def _refresh_shadows_now(self):
        """refresh_weight_shadows() for the cached paths, which then read every shadow at once: a recast it queued on the side stream (UDM_OVERLAP_CAST)
        is awaited here, before any decode or prefill launch."""
        self.refresh_weight_shadows()
        for key in list(getattr(self, "_cast_events", {})):
            self._await_cast(key)

    def _rope_rows(self, p):
        """rotary rows of decode position p: (cos, sin) with the qk-norm + rope kernel's table form (a one-row table, or [1, Bp, D/2] per row)"""
        kv = self._kv
        if kv.cos is None:
            return self.rotary_cos_emb[p:p + 1], self.rotary_sin_emb[p:p + 1]
        return kv.cos[p][None], kv.sin[p][None]

    @torch.no_grad()
    def _decode_step(self, p):
        """One token per cached row at position p (the ids in self._kv.ids) -> logits [Bp, Vp] bf16 (self._kv.logits).  Engine path without autograd or host
        synchronisation: norm, skinny qkv, qk-norm + rope (row p of the full-length tables), decode attention (appends k / v at slot p), skinny out-proj,
        residual + norm, skinny up + GELU, skinny down, residual (+ the next block's norm), head."""
        kv = self._kv
        emb_mod = kv.mod_cols[p] if (self.modality_embed is not None) else None
        cos, sin = self._rope_rows(p)
        self._decode_launches(emb_mod, cos, sin, p)
        kv.pos = p + 1
        return kv.logits

    @torch.no_grad()
    def _decode_step_at(self):
        """_decode_step at the position held in self._kv.pos_dev (device memory, read by the kernels): the same launches on fixed operands - one gather of
        the position's modality column and rotary rows into one-row buffers (udm_decode_stage), attention through udm_attention_decode_at.  No host
        position, no allocation, no read of the device: the sequence a graph captures once and replays for every token (capture_decode_step).  The
        caller keeps self._kv.pos in step (the host cannot know the device's position)."""
        kv = self._kv
        K.decode_stage(kv.pos_dev, mod_cols=kv.mod_cols if kv.mod_row is not None else None, mod_row=kv.mod_row, cos=kv.rope_tabs[0], sin=kv.rope_tabs[1],
                       cos_row=kv.cos_row, sin_row=kv.sin_row)
        self._decode_launches(kv.mod_row, kv.cos_row, kv.sin_row, None)
        return kv.logits

    def _decode_launches(self, emb_mod, cos, sin, p):
        """the launches of a decode step behind its position-dependent operands; p None: the attention reads the position from self._kv.pos_dev"""
        kv, lin = self._kv, self._lins
        d, H, D = self.hidden_size, self.n_heads, self.head_dim
        nt = K.norm_id(self.norm_type)
        sw = self.sandwich_normalization
        xa, xb = kv.x
        st = kv.stat
        K.embedding_fwd(kv.ids, self.vocab_embed.embedding.detach(), emb_mod, self.modality_embed.embedding.detach() if self.modality_embed is not None else None,
                        out=xa)
        res_out = (None, st[0], st[1], kv.h, st[2], st[3])
        for i, blk in enumerate(self.blocks):
            if i == 0:
                K.norm_fwd(xa, blk.norm1.weight.detach(), nt, 1, out=(kv.h, st[2], st[3]))
            qkv = K.gemm_skinny(kv.h, lin[f"{i}.qkv"].w16, out=kv.qkv, N=3 * d, ws=kv.gws)
            at = blk.attention
            qn_kw = dict(gq=at.q_norm.weight.detach(), bq=at.q_norm.bias.detach(), gk=at.k_norm.weight.detach(), bk=at.k_norm.bias.detach()) if self.qk_norm else {}
            qkr, _ = K.qknorm_rope_fwd(qkv, cos, sin, 1, D, q_scale=self.attn_q_scale, out=(kv.qkr, kv.qstats), **qn_kw)
            if p is None:
                o = K.attention_decode_at(qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], kv.K[i], kv.V[i], kv.pos_dev, H, D, out=kv.o, ws=kv.aws)
            else:
                o = K.attention_decode(qkr[:, :d], qkr[:, d:], qkv[:, 2 * d:], kv.K[i], kv.V[i], p, H, D, out=kv.o, ws=kv.aws)
            a_out = K.gemm_skinny(o, lin[f"{i}.out"].w16, out=kv.a_out, N=d, ws=kv.gws)
            K.residual_fwd(xa, a_out, 1, w_b=blk.pre_residual_norm.weight.detach() if sw else None, norm_type=nt, next_w=blk.norm2.weight.detach(),
                           out=(xb,) + res_out[1:])
            f1, f2 = lin[f"{i}.fc1"], lin[f"{i}.fc2"]
            g = K.gemm_skinny(kv.h, f1.w16, out=kv.g, N=4 * d, epilogue=K.EPI_BIAS_GELU, bias=f1.bias.detach(), ws=kv.gws)
            u2 = K.gemm_skinny(g, f2.w16, out=kv.u2, N=d, epilogue=K.EPI_BIAS, bias=f2.bias.detach(), ws=kv.gws)
            nxt_w = (self.blocks[i + 1].norm1.weight if i + 1 < self.n_blocks else self.output_layer.norm_final.weight).detach()
            K.residual_fwd(xb, u2, 1, w_b=blk.post_ff_norm.weight.detach() if sw else None, norm_type=nt, next_w=nxt_w, out=(xa,) + res_out[1:])
        head = lin["head"]
        K.gemm_skinny(kv.h, head.w16, out=kv.logits, N=self.vocab_size, epilogue=K.EPI_BIAS, bias=head.bias.detach(), ws=kv.gws)

    def set_decode_position(self, p):
        """the position the next _decode_step_at / replay works at: a device-side fill of self._kv.pos_dev, no host read (after a prefill or a chunk: p =
        the number of cache slots written)"""
        kv = self._kv
        kv.pos = int(p)
        kv.pos_dev.fill_(int(p))

    def capture_decode_step(self, tail=None):
        """Capture `_decode_step_at(); tail(); pos_dev += 1` into one graph and return it: `replay()` is then one graph launch per token, whatever the
        position.  tail: the token choice on self._kv.logits, through the device-position forms (K.ar_sample_rows_at / K.ar_nucleus_rows_at on
        self._kv.pos_dev), writing the next input ids into self._kv.ids.  The sequence runs once eagerly first (first launches, any lazy allocation); that
        run is undone - self._kv.ids and the position are put back, and what else it wrote (cache slot p, the tail's outputs) the first replay writes again
        with the same values, since every launch is deterministic in (ids, position).  The weight shadows are refreshed and any recast queued on the side
        stream is awaited before, so the capture holds launches of one stream only: one linear chain.  A capture the runtime rejects raises RuntimeError
        naming the launch; there is no eager fallback."""
        kv = self._kv
        if kv is None:
            raise RuntimeError("unidisc_amd.DIT.capture_decode_step: no KV cache - call reset_kv_cache(batch_size, seq_len, ...) first")
        self._refresh_shadows_now()
        return _DecodeGraph(self, tail)

    @torch.no_grad()
    def _prefill(self, ids, modality=None, last_only=False):
        """start_pos = 0 over n >= 1 tokens of every cached row: the causal forward (rotary rows 0..n-1 of the full-length tables) that leaves each block's
        post-rope k and v in cache slots [0, n).  ids / modality [B, n] with B <= the cached rows (padded with row 0).  Returns logits [B, n, V], or with
        last_only the logits of position n - 1 in self._kv.logits [Bp, Vp]."""
        kv = self._kv
        B, n = ids.shape
        if n > kv.Lmax:
            raise ValueError(f"unidisc_amd.DIT: prefill of {n} tokens into a cache of {kv.Lmax}")
        Bp = kv.Bp
        pad = lambda t: torch.cat([t, t[:1].expand(Bp - B, *t.shape[1:])], 0) if (t is not None and Bp > B) else t   # noqa: E731
        idsp = pad(ids.to(torch.int64)).contiguous()
        mod = modality.to(torch.int64) if modality is not None else (kv.mod_full[:B, :n] if kv.mod_full is not None else None)
        modp = pad(mod).contiguous() if mod is not None else None
        rope = None
        if kv.cos is not None:
            rope = (kv.cos[:n].transpose(0, 1).contiguous(), kv.sin[:n].transpose(0, 1).contiguous())
        inputs = _EngineInputs(indices=idsp, modality=modp, kv_sink=list(zip(kv.K, kv.V)), rope=rope, head_out=kv.logits if last_only else None)
        out, _ = self._engine_forward(inputs, "logits", save=False)
        kv.pos = n
        return out if last_only else out[:B]

    @torch.no_grad()
    def _forward_chunk(self, ids, modality, p, last_only=False):
        """start_pos = p > 0 over n >= 1 tokens of every cached row (chunked prefill): the engine's ordinary forward on the n positions p .. p + n - 1 - rotary
        rows and modality columns p .. p + n - 1 of the full-length tables - whose attention writes this call's post-rope k and v into cache slots [p, p + n)
        and lets query i see the slots [0, p + i] (udm_attention_fwd_kv_causal).  The slots [0, p) must have been written (p <= self._kv.pos: the caller's
        check).  ids / modality [B, n], rows padded with row 0 as in _prefill.  Returns logits [B, n, V], or with last_only the logits of position p + n - 1
        in self._kv.logits [Bp, Vp]; self._kv.pos = p + n."""
        kv = self._kv
        B, n = ids.shape
        Bp = kv.Bp
        pad = lambda t: torch.cat([t, t[:1].expand(Bp - B, *t.shape[1:])], 0) if (t is not None and Bp > B) else t   # noqa: E731
        idsp = pad(ids.to(torch.int64)).contiguous()
        mod = modality.to(torch.int64) if modality is not None else (kv.mod_full[:B, p:p + n] if kv.mod_full is not None else None)
        modp = pad(mod).contiguous() if mod is not None else None
        if kv.cos is not None:
            rope = (kv.cos[p:p + n].transpose(0, 1).contiguous(), kv.sin[p:p + n].transpose(0, 1).contiguous())
        else:
            rope = (self.rotary_cos_emb[p:p + n].contiguous(), self.rotary_sin_emb[p:p + n].contiguous())
        inputs = _EngineInputs(indices=idsp, modality=modp, kv_read=_KVRead(K=kv.K, V=kv.V, slot0=p, Lk=p + n, causal=True), rope=rope,
                               head_out=kv.logits if last_only else None)
        out, _ = self._engine_forward(inputs, "logits", save=False)
        kv.pos = p + n
        return out if last_only else out[:B]

    def set_flex_attention_cache(self, batch_size=None, seq_len=None, device=None, dtype=None, read_cache=False):
        """read_cache (extension, eval.attention_caching_read_cache): allocate per block bf16 K / V [batch_size, seq_len, d] (2 GB at 1.4 B, B = 8) that the
        build step fills (every position's post-rope k and its v) and the text steps read: forward_masked_logits(modality_cache="build" / "read")."""
        self.use_flex_attention_cache = True
        self._mc = None
        if not read_cache:
            return
        if self.time_conditioning:
            raise NotImplementedError("unidisc_amd.DIT.set_flex_attention_cache(read_cache=True): with time_conditioning the cached image keys would depend on sigma")
        if self.causal or self.require_sample_ids:
            raise NotImplementedError("unidisc_amd.DIT.set_flex_attention_cache(read_cache=True): built for bidirectional backbones on unpacked batches")
        sl = self.static_txt_sl
        if self.txt_length <= 0 or self.img_length <= 0 or (sl is not None and ((sl.start or 0) != 0 or sl.stop != self.txt_length or sl.step not in (None, 1))):
            raise NotImplementedError("unidisc_amd.DIT.set_flex_attention_cache(read_cache=True): the text must be the static slice [:txt_length] of the sequence "
                                      f"(static_txt_sl = {sl}, txt_length = {self.txt_length}, img_length = {self.img_length})")
        B, L = int(batch_size), int(seq_len)
        if L != self.total_length:
            raise ValueError(f"unidisc_amd.DIT.set_flex_attention_cache(read_cache=True): seq_len {L} is not model.length = {self.total_length}")
        dev = torch.device(device) if device is not None else self.vocab_embed.embedding.device
        mc = types.SimpleNamespace(B=B, L=L, Lt=int(self.txt_length), built=False, cos=None, sin=None, mod=None)
        mc.K = [torch.zeros((B, L, self.hidden_size), dtype=BF16, device=dev) for _ in self.blocks]
        mc.V = [torch.zeros((B, L, self.hidden_size), dtype=BF16, device=dev) for _ in self.blocks]
        self._mc = mc

    def set_conditioning_cache(self, batch_size, seq_len, device=None, given="text", guided=False):
        """Conditional sampling (extension, eval.conditioning_cache): one modality of every sample - `given`, "text" = positions [:txt_length] or "image" = the rest
        - is fixed for the whole run.  Under the ModalityMask that blinds the given modality's queries to the other modality (txt_drop = 1 / img_drop = 1) its
        hidden states, and so its K / V in every block, are a function of its own tokens alone: constant over the run, and constant ([MASK] everywhere) in the
        unconditional half of guided sampling.  Allocates per block bf16 K / V [R, seq_len, d] (R = 2 batch_size with `guided`: rows [0, B) the conditional half,
        [B, 2 B) the unconditional one) and the split workspace of udm_attention_fwd_kv_split; forward_masked_logits(conditioning_cache="build") fills them with
        one full-length forward, every conditioning_cache="read" forward then runs on the generated slice alone.  Nothing goes stale: what is cached never
        changes.  reset_kv_cache() frees it."""
        self._cc = None
        name = "unidisc_amd.DIT.set_conditioning_cache"
        if given not in ("text", "image"):
            raise ValueError(f"{name}: given={given!r} (\"text\" or \"image\")")
        if self.time_conditioning:
            raise NotImplementedError(f"{name}: with time_conditioning the cached conditioning keys would depend on sigma")
        if self.causal or self.require_sample_ids:
            raise NotImplementedError(f"{name}: built for bidirectional backbones on unpacked batches")
        sl = self.static_txt_sl
        if self.txt_length <= 0 or self.img_length <= 0 or (sl is not None and ((sl.start or 0) != 0 or sl.stop != self.txt_length or sl.step not in (None, 1))):
            raise NotImplementedError(f"{name}: the text must be the static slice [:txt_length] of the sequence "
                                      f"(static_txt_sl = {sl}, txt_length = {self.txt_length}, img_length = {self.img_length})")
        B, L = int(batch_size), int(seq_len)
        if L != self.total_length:
            raise ValueError(f"{name}: seq_len {L} is not model.length = {self.total_length}")
        dev = torch.device(device) if device is not None else self.vocab_embed.embedding.device
        Lt = int(self.txt_length)
        R = 2 * B if guided else B
        cc = types.SimpleNamespace(B=B, R=R, L=L, Lt=Lt, given=given, guided=bool(guided), built=set(), sliced={}, cos=None, sin=None, mod=None)
        cc.sl = slice(Lt, L) if given == "text" else slice(0, Lt)      # the generated slice: what a read step runs on, and the cache slots it rewrites
        cc.Lq = cc.sl.stop - cc.sl.start
        cc.K = [torch.zeros((R, L, self.hidden_size), dtype=BF16, device=dev) for _ in self.blocks]
        cc.V = [torch.zeros((R, L, self.hidden_size), dtype=BF16, device=dev) for _ in self.blocks]
        # one workspace for the pass over all R rows and for the two passes of B rows (eval.split_cfg_batches), whose plan may split further
        need = max(K.attention_kv_split_plan(rows, cc.Lq, L, self.n_heads, self.head_dim)[1] for rows in {R, B})
        cc.ws = torch.empty(need, dtype=F32, device=dev) if need > 0 else None
        self._cc = cc

    # -------------------------------------------------------------------------------------------- parameters / shadows
    IMG_BLOCKS = ((256, 1), (1024, 2), (2304, 3), (4096, 4))   # (tokens of an image block, Lumina linear factor), models/dit.py:1210

    def _ordered_params(self) -> List[nn.Parameter]:
        """Parameters in the order their gradients become final during backward (head first, embeddings last)."""
        out = list(self.output_layer.parameters())
        for blk in reversed(self.blocks):
            out += list(blk.parameters())
        out += list(self.vocab_embed.parameters())
        if self.modality_embed is not None:
            out += list(self.modality_embed.parameters())
        if getattr(self, "img_count_embedding", None) is not None:
            out.append(self.img_count_embedding)
        if self.sigma_map is not None:
            out += list(self.sigma_map.parameters())
        seen = {id(p) for p in out}
        assert len(seen) == len(out) == sum(1 for _ in self.parameters())
        return out

    def _build_lins(self):
        L: Dict[str, _Lin] = {}
        for i, blk in enumerate(self.blocks):
            L[f"{i}.qkv"] = _Lin(blk.attention.attn_qkv.weight, None)
            L[f"{i}.out"] = _Lin(blk.attention.attn_out.weight, None)
            L[f"{i}.fc1"] = _Lin(blk.mlp[0].weight, blk.mlp[0].bias)
            L[f"{i}.fc2"] = _Lin(blk.mlp[2].weight, blk.mlp[2].bias)
            if self.time_conditioning:
                L[f"{i}.ada"] = _Lin(blk.adaLN_modulation.weight, blk.adaLN_modulation.bias)
        L["head"] = _Lin(self.output_layer.linear.weight, self.output_layer.linear.bias, out_pad=128)
        if self.time_conditioning:
            L["head.ada"] = _Lin(self.output_layer.adaLN_modulation.weight, self.output_layer.adaLN_modulation.bias)
            L["sig0"] = _Lin(self.sigma_map.mlp[0].weight, self.sigma_map.mlp[0].bias)
            L["sig2"] = _Lin(self.sigma_map.mlp[2].weight, self.sigma_map.mlp[2].bias)
        self._lins = L

    def refresh_weight_shadows(self, force=False, rows=None):
        if self._lins is None or next(iter(self._lins.values())).weight.device != self.vocab_embed.embedding.device:
            self._build_lins()
            force = True
        if rows is not None and self.dgrad_from_w and next(iter(self._lins.values())).weight.is_cuda:
            # qkv / out-proj / mlp.0 dgrads read W itself (K.gemm_nn) where `rows` x in x out are whole tiles of that kernel: their transposed
            # shadows - a quarter of the per-step cast traffic - are then not produced.  (mlp.2's dgrad carries the GELU' epilogue and the last
            # block may run on a compacted row list: they keep the transposed shadow.)
            last = len(self.blocks) - 1
            for name, lin in self._lins.items():
                blk, _, kind = name.partition(".")
                want_t = not (kind in ("qkv", "out", "fc1") and not (self.compact_last_block and int(blk) == last) and K.gemm_nn_ok(rows, lin.inp, lin.out))
                # sticky: once some forward needed the transposed shadow it stays (a second forward with another row count - micro-batches, an eval pass inside
                # a training step - must not drop the shadow a still-pending backward dispatches on, nor force a full recast at every alternation)
                lin.sticky_t = lin.sticky_t or want_t
                want_t = lin.sticky_t
                if want_t != lin.need_t:
                    lin.need_t, force = want_t, True
        versions = [l.weight._version for l in self._lins.values()]
        self._cast_events = {}
        if force or self.recast_every_forward and self.training or versions != self._shadow_versions:
            groups: Dict[str, list] = {}
            for name, lin in self._lins.items():   # "pre" (timestep MLP), one group per block in forward order, "head"
                key = "pre" if name.startswith("sig") else ("head" if name.startswith("head") else name.split(".")[0])
                groups.setdefault(key, []).append(lin)
            order = [k for k in ["pre"] + [str(i) for i in range(len(self.blocks))] + ["head"] if k in groups]
            dev = self.vocab_embed.embedding.device
            if self.overlap_weight_cast and dev.type == "cuda" and not force:
                # Opt-in (UDM_OVERLAP_CAST=1): the casts are HBM-bound and the GEMMs they feed are not, so all but the first blocks' shadows are
                # refreshed on a side stream under the forward of the blocks before them: a few multi-matrix launches (first two blocks /
                # next quarter / the rest + head); the compute stream waits for a group right before its first block (_await_cast).
                if getattr(self, "_cast_stream", None) is None:
                    self._cast_stream = torch.cuda.Stream(device=dev)
                side, main = self._cast_stream, torch.cuda.current_stream(dev)
                nb = len(self.blocks)
                cuts = [0, min(2, nb), min(max(nb // 3, 2), nb), nb]
                bounds = sorted(set(cuts))
                parts = []
                for lo_b, hi_b in zip(bounds[:-1], bounds[1:]):
                    keys = [str(i) for i in range(lo_b, hi_b)]
                    if lo_b == 0:
                        keys = ["pre"] + keys
                    if hi_b == nb:
                        keys = keys + ["head"]
                    parts.append([k for k in keys if k in groups])
                for lins_k in parts:
                    for k in lins_k:
                        for lin in groups[k]:
                            lin.alloc()
                key = tuple((l.weight.data_ptr(), l.w16.data_ptr(), l.w16t.data_ptr() if l.w16t is not None else 0) for k in order for l in groups[k])
                if getattr(self, "_cast_parts_key", None) != key:
                    self._cast_parts = [K.cast_transpose_jobs([(l.weight.detach(), l.w16, l.w16t) for k in ks for l in groups[k]], dev) for ks in parts]
                    self._cast_parts_key = key
                side.wait_stream(main)   # everything enqueued so far (the previous backward reads the Wᵀ shadows) comes first
                with torch.cuda.stream(side):
                    for ks, jobs in zip(parts, self._cast_parts):
                        K.cast_transpose_multi(jobs)
                        ev = torch.cuda.Event()
                        ev.record(side)
                        self._cast_events[ks[0]] = ev
            else:
                # every weight of the forward in ONE launch (97 at 1.4 B): the job table lives on the device and is rebuilt only when a
                # master weight or a shadow moved
                lins = [lin for k in order for lin in groups[k]]
                for lin in lins:
                    lin.alloc()
                key = tuple((l.weight.data_ptr(), l.w16.data_ptr(), l.w16t.data_ptr() if l.w16t is not None else 0) for l in lins)
                if getattr(self, "_cast_jobs_key", None) != key:
                    self._cast_jobs = K.cast_transpose_jobs([(l.weight.detach(), l.w16, l.w16t) for l in lins], dev)
                    self._cast_jobs_key = key
                K.cast_transpose_multi(self._cast_jobs)
            self._shadow_versions = versions

    def invalidate_shadows(self):
        """Force the next forward to rebuild the bf16 weight shadows.  Needed after any write to the master weights that does not bump tensor
        versions (collectives, ``p.data`` writes, kernels called through ctypes, optimizer state reloads)."""
        self._shadow_versions = None

    @staticmethod
    def _dropout_rank():
        """Data-parallel ranks seeded identically must still draw different dropout masks (torch's CUDA generator differs per process in the
        reference because every rank seeds with seed + rank, main.py:1058-1068; here the rank is mixed in explicitly)."""
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def _await_cast(self, key):
        ev = self._cast_events.pop(str(key), None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    # -------------------------------------------------------------------------------------------- public forward
    def forward(self, indices, sigma=None, label=None, x_cond=None, attention_mask=None, continuous_mode=False, x_img_emb=None, modality=None,
                start_pos=None, block_mask=None, update_cache_slice=None, sample_ids=None):
        """→ logits [B, L, V] (bf16).  Signature of the reference's DIT.forward (models/dit.py:1324-1338)."""
        self._check_unsupported(label, x_cond, None, continuous_mode, x_img_emb, None, block_mask, update_cache_slice, sample_ids)
        if start_pos is not None:
            return self._forward_cached(indices, modality, int(start_pos), attention_mask, block_mask)
        params = self._ordered_params()
        inputs = _EngineInputs(indices=indices, sigma=sigma, modality=modality, sample_ids=sample_ids, save=self._needs_grad(params),
                               block_mask=block_mask if isinstance(block_mask, ModalityMask) else None, key_mask=self._key_mask(attention_mask, indices))
        return _DitFn.apply(self, "logits", inputs, *params)

    @torch.no_grad()
    def _forward_cached(self, indices, modality, start_pos, attention_mask, block_mask):
        """forward(start_pos=p) on the KV cache (reset_kv_cache first), the reference's models/dit.py:1324-1338 with :776-780: n >= 1 tokens at p = 0 (prefill,
        logits [B, n, V]), one token per row at p > 0 (the decode step, logits [B, 1, V]), or n > 1 tokens at p > 0 (a chunk: the engine's forward over the
        cache, _forward_chunk, logits [B, n, V]).  A chunk or a step may start at any p <= the number of slots written so far (rewriting slots is allowed,
        leaving a gap is not) and must end inside the cache.  HIP kernels only: CPU tensors are refused before anything else is looked at."""
        if self._kv is None:
            raise RuntimeError("unidisc_amd.DIT.forward(start_pos=...): no KV cache - call reset_kv_cache(batch_size, seq_len, ...) first")
        if attention_mask is not None or (block_mask is not None and block_mask is not True):
            raise NotImplementedError("unidisc_amd.DIT.forward(start_pos=...): the KV-cached forward takes no attention_mask / block_mask")
        kv = self._kv
        B, n = indices.shape
        if B > kv.B:
            raise ValueError(f"unidisc_amd.DIT.forward(start_pos=...): {B} rows, the cache holds {kv.B}")
        if start_pos == 0:
            K.require_gpu(indices)
            return self._prefill(indices, modality)
        if n != 1:
            if not indices.is_cuda:   # (first: nothing else of the cache is read for a call that cannot run)
                raise NotImplementedError(f"unidisc_amd.DIT.forward: start_pos={start_pos} with {n} tokens runs on HIP kernels; there is no CPU path")
            if start_pos < 0 or start_pos + n > kv.Lmax:
                raise ValueError(f"unidisc_amd.DIT.forward: start_pos={start_pos} with {n} tokens outside the cache [0, {kv.Lmax})")
            if start_pos > kv.pos:
                raise ValueError(f"unidisc_amd.DIT.forward: start_pos={start_pos} with {n} tokens, but only the slots [0, {kv.pos}) are written - "
                                 "the chunk would attend to slots nobody filled")
            return self._forward_chunk(indices, modality, start_pos)
        if not 0 < start_pos < kv.Lmax:
            raise ValueError(f"unidisc_amd.DIT.forward: start_pos={start_pos} outside the cache [0, {kv.Lmax})")
        K.require_gpu(indices)
        self._refresh_shadows_now()
        kv.ids[:B].copy_(indices[:, 0])
        if modality is not None and kv.mod_cols is not None:   # (the step's own modality column, when given, for the embedding)
            kv.mod_cols[start_pos, :B].copy_(modality[:, 0])
        logits = self._decode_step(start_pos)
        return logits[:B, :self.vocab_size].view(B, 1, self.vocab_size)

    @staticmethod
    def _key_mask(attention_mask, indices):
        """`model.use_attention_mask` (model.py:405-406 -> `sdpa(..., attn_mask=attention_mask)`, models/dit.py:829): the batch's [B, L] bool mask reaches SDPA
        unchanged, where a 2-D mask aligns with the (query, key) axes - i.e. it broadcasts (B = 1; for B > 1 the reference call does not broadcast and
        fails) as a KEY mask: padded keys are hidden from every query of their sample, padded queries still attend to the valid keys."""
        if attention_mask is None:
            return None
        if attention_mask.dtype != torch.bool or tuple(attention_mask.shape) != tuple(indices.shape):
            raise NotImplementedError("unidisc_amd.DIT.forward: attention_mask must be the batch's bool [B, L] padding mask (dense [B, 1, L, L] masks - the "
                                      "transfusion path - are outside the denoising hot path)")
        return attention_mask

    def forward_logp(self, xt, x0, sigma=None, modality=None, sample_ids=None, restrict_modality=False, block_mask=None, attention_mask=None, ar_shift=False):
        """Fused training path: log p_theta(x0 | xt) per token [B, L] fp32 under the SUBS parameterisation
        (== gather(_subs_parameterization(logits, xt), x0), model.py:621-658 + :967) without materialising log-probs.
        block_mask: a `ModalityMask` (modality attention dropout) or None.  attention_mask: the key-padding mask of `model.use_attention_mask` or None.
        ar_shift (the AR baseline, model.py:717-781 + :935-967; pass xt = x0): column r of the result is log p(x0[:, r+1] | x0[:, :r+1]) - the [MASK] id and,
        with restrict_modality, the ids of the other modality than the TARGET's excluded - and the last column, which has no target, is 0 (zero gradient)."""
        params = self._ordered_params()
        inputs = _EngineInputs(indices=xt, sigma=sigma, modality=modality, sample_ids=sample_ids, x0=x0, restrict=bool(restrict_modality),
                               save=self._needs_grad(params), block_mask=block_mask, key_mask=self._key_mask(attention_mask, xt), ar_shift=bool(ar_shift))
        return _DitFn.apply(self, "logp", inputs, *params)

    @torch.no_grad()
    def forward_masked_logits(self, xt, sigma=None, modality=None, sample_ids=None, plan_ids=None, block_mask=None, modality_cache=None, conditioning_cache=None,
                              cache_row0=0):
        """Sampler path: (logits [R, Vp] bf16 of the [MASK] positions of `xt` first, then padding rows; their flat row indices [R];
        the number of [MASK] rows).  Unmasked positions keep their token under SUBS (model.py:646-656), so they need no logits.
        `plan_ids` (same shape as xt): take the row selection from the [MASK] positions of this tensor instead of xt's (guided sampling runs
        [x ; x_uncond] as one batch and needs the SAME positions from both halves).
        `modality_cache` (set_flex_attention_cache(read_cache=True) first): "build" - a full-length forward (the caller passes the image-queries-see-image-keys
        ModalityMask) that also leaves every block's post-rope k and its v of all L positions in the cache; "read" - xt is the text slice [B, txt_length]: the
        backbone runs on those rows alone, with the modality ids and rotary rows of the full-length forward, writes their k / v into cache slots [0, txt_length)
        and attends to [fresh text keys ; cached image keys] (udm_attention_fwd_kv).  Under the build step's mask the image rows never see a text key, so their
        K / V depend on the image tokens alone: a "read" step equals the text rows of the masked full-length forward on [xt ; image tokens of the build step].
        `conditioning_cache` (set_conditioning_cache first; conditional sampling, see there): "build" - a full-length forward under the ModalityMask that blinds
        the GIVEN modality's queries to the other one (built here), leaving every block's post-rope k and its v in cache rows [cache_row0, cache_row0 + rows of
        xt); "read" - xt is the generated slice: the backbone runs on those rows alone with the modality ids and rotary rows of the build step's tables, writes
        their k / v into the slice's cache slots and attends to all L slots (udm_attention_fwd_kv_split).  A read step equals the generated rows of that masked
        full-length forward on [given ; xt].  `plan_ids` is accepted (the two halves of guided sampling need the same positions); xt holds either all cache rows
        ([x ; x_uncond]) or, with cache_row0 = 0 / B, one half (eval.split_cfg_batches: two passes, each on its half of the cache)."""
        if conditioning_cache is not None:
            if modality_cache is not None:
                raise ValueError("unidisc_amd.DIT.forward_masked_logits: modality_cache and conditioning_cache are two different caches - pass one")
            return self._conditioning_forward(xt, sigma, modality, sample_ids, plan_ids, block_mask, conditioning_cache, int(cache_row0))
        inputs = _EngineInputs(indices=xt, sigma=sigma, modality=modality, sample_ids=sample_ids, plan_ids=plan_ids,
                               block_mask=block_mask if isinstance(block_mask, ModalityMask) else None)
        mc = self._mc
        if modality_cache is not None:
            if modality_cache not in ("build", "read"):
                raise ValueError(f"unidisc_amd.DIT.forward_masked_logits: modality_cache={modality_cache!r} (\"build\", \"read\" or None)")
            if mc is None:
                raise RuntimeError("unidisc_amd.DIT.forward_masked_logits(modality_cache=...): no modality cache - call set_flex_attention_cache(B, L, device, dtype, "
                                   "read_cache=True) first")
            if sample_ids is not None or plan_ids is not None or sigma is not None and self.time_conditioning:
                raise NotImplementedError("unidisc_amd.DIT.forward_masked_logits(modality_cache=...): no packed sample ids, guidance halves or time conditioning")
            B, Lx = xt.shape
            if B != mc.B or Lx != (mc.L if modality_cache == "build" else mc.Lt):
                raise ValueError(f"unidisc_amd.DIT.forward_masked_logits(modality_cache={modality_cache!r}): xt {tuple(xt.shape)}, the cache serves "
                                 f"[{mc.B}, {mc.L}] with {mc.Lt} text positions")
        if modality_cache == "build":
            inputs.kv_sink = list(zip(mc.K, mc.V))
            out, S = self._engine_forward(inputs, "rows", save=False)
            mc.cos, mc.sin = S.cos, S.sin                                         # the full-length rotary tables ([L, D/2], or per sample [B, L, D/2])
            mc.mod = modality.to(torch.int64).contiguous() if modality is not None else None
            mc.built = True
            return out
        if modality_cache == "read":
            if not mc.built:
                raise RuntimeError("unidisc_amd.DIT.forward_masked_logits(modality_cache=\"read\"): the cache holds no image keys yet (no \"build\" step ran)")
            Lt = mc.Lt
            if mc.mod is not None:   # row p takes exactly the modality id and the rotary row of the full-length forward
                inputs.modality = mc.mod[:, :Lt].contiguous()
            inputs.rope = (mc.cos[..., :Lt, :].contiguous(), mc.sin[..., :Lt, :].contiguous())
            inputs.kv_read = _KVRead(K=mc.K, V=mc.V, slot0=0, Lk=mc.L)
        return self._engine_forward(inputs, "rows", save=False)[0]

    def _conditioning_forward(self, xt, sigma, modality, sample_ids, plan_ids, block_mask, what, row0):
        name = f"unidisc_amd.DIT.forward_masked_logits(conditioning_cache={what!r})"
        cc = self._cc
        if what not in ("build", "read"):
            raise ValueError(f"{name}: \"build\", \"read\" or None")
        if cc is None:
            raise RuntimeError(f"{name}: no conditioning cache - call set_conditioning_cache(B, L, device, given=..., guided=...) first")
        if sample_ids is not None or block_mask is not None or sigma is not None and self.time_conditioning:
            raise NotImplementedError(f"{name}: no packed sample ids, no caller's block mask (the build step makes its own), no time conditioning")
        rows, Lx = xt.shape
        if Lx != (cc.L if what == "build" else cc.Lq) or row0 < 0 or row0 + rows > cc.R or (rows != cc.R and (rows != cc.B or row0 % cc.B != 0)):
            raise ValueError(f"{name}: xt {tuple(xt.shape)} at cache row {row0}; the cache serves {cc.R} rows of length {cc.L}, in passes of {cc.R} or {cc.B} rows, "
                             f"with a generated slice of {cc.Lq} positions")
        dev = xt.device
        inputs = _EngineInputs(indices=xt, sigma=sigma, modality=modality, plan_ids=plan_ids)
        span = range(row0, row0 + rows)
        if what == "build":
            on = torch.ones(rows, dtype=torch.bool, device=dev)
            inputs.block_mask = ModalityMask(on if cc.given == "text" else ~on, on if cc.given == "image" else ~on, cc.Lt)
            inputs.kv_sink = [(k[row0:row0 + rows], v[row0:row0 + rows]) for k, v in zip(cc.K, cc.V)]
            out, S = self._engine_forward(inputs, "rows", save=False)
            cos, sin = S.cos, S.sin                      # [L, D/2], or per sample [rows, L, D/2]
            if cos.dim() == 3:                           # per-sample tables: kept per cache row
                if cc.cos is None or cc.cos.dim() != 3:
                    cc.cos, cc.sin = cos.new_zeros((cc.R,) + tuple(cos.shape[1:])), sin.new_zeros((cc.R,) + tuple(sin.shape[1:]))
                cc.cos[row0:row0 + rows], cc.sin[row0:row0 + rows] = cos, sin
            else:
                cc.cos, cc.sin = cos, sin
            mod = modality.to(torch.int64) if modality is not None else (self._static_modality(rows, cc.L, dev) if self.modality_embed is not None else None)
            if mod is not None:
                if cc.mod is None:
                    cc.mod = torch.zeros((cc.R, cc.L), dtype=torch.int64, device=dev)
                cc.mod[row0:row0 + rows] = mod
            cc.built.update(span)
            cc.sliced.clear()
            return out
        if not set(span) <= cc.built:
            raise RuntimeError(f"{name}: the cache holds no conditioning keys for rows [{row0}, {row0 + rows}) yet (no \"build\" step ran on them)")
        sl = cc.sl
        if (row0, rows) not in cc.sliced:   # row p takes exactly the modality id and the rotary row of the full-length forward (cut once: they never change)
            pick = (lambda t: t[row0:row0 + rows, sl].contiguous()) if cc.cos.dim() == 3 else (lambda t: t[sl].contiguous())
            cc.sliced[(row0, rows)] = (None if cc.mod is None else cc.mod[row0:row0 + rows, sl].contiguous(), pick(cc.cos), pick(cc.sin))
        mod_sl, cos_sl, sin_sl = cc.sliced[(row0, rows)]
        if mod_sl is not None:
            inputs.modality = mod_sl
        inputs.rope = (cos_sl, sin_sl)
        inputs.kv_read = _KVRead(K=[k[row0:row0 + rows] for k in cc.K], V=[v[row0:row0 + rows] for v in cc.V], slot0=sl.start, Lk=cc.L, split=True, ws=cc.ws)
        return self._engine_forward(inputs, "rows", save=False)[0]

    @staticmethod
    def _needs_grad(params):
        return torch.is_grad_enabled() and any(p.requires_grad for p in params)

    def _check_unsupported(self, label, x_cond, attention_mask, continuous_mode, x_img_emb, start_pos, block_mask, update_cache_slice, sample_ids):
        for name, v in (("label", label), ("x_cond", x_cond), ("attention_mask", attention_mask), ("x_img_emb", x_img_emb), ("start_pos", start_pos),
                        ("update_cache_slice", update_cache_slice)):
            if v is not None:
                raise NotImplementedError(f"unidisc_amd.DIT.forward: argument `{name}` is outside the denoising hot path")
        if continuous_mode:
            raise NotImplementedError("unidisc_amd.DIT.forward: continuous_mode is outside the denoising hot path")
        if block_mask is not None and block_mask is not True and sample_ids is None and not isinstance(block_mask, ModalityMask):
            raise NotImplementedError("unidisc_amd.DIT.forward: pass a unidisc_amd.ModalityMask (modality attention dropout) as block_mask; "
                                      "FlexAttention BlockMask objects are not used here (document masks are derived from sample_ids)")

    # -------------------------------------------------------------------------------------------- engine: forward
    def _rotary_interleaved(self, modality, sample_ids):
        """Rotary rows and image-count indices of packed rows: ONE launch on the GPU (`udm_interleaved_rope`, tokens.hip), the tensor-statement form below elsewhere
        (CPU tests) - bit-identical (tests/test_gpu_kernels.py)."""
        if modality.is_cuda and os.environ.get("UDM_INTERLEAVED_KERNELS", "1") != "0":
            dev = modality.device
            if getattr(self, "_img_tab_cos", None) is None or self._img_tab_cos.device != dev:
                self._img_tab_cos = torch.cat([getattr(self, f"rotary_cos_emb_img_{n}") for n, _ in self.IMG_BLOCKS], 0).to(dev).contiguous()
                self._img_tab_sin = torch.cat([getattr(self, f"rotary_sin_emb_img_{n}") for n, _ in self.IMG_BLOCKS], 0).to(dev).contiguous()
            return K.interleaved_rope(modality, sample_ids, self._img_tab_cos, self._img_tab_sin, [n for n, _ in self.IMG_BLOCKS],
                                      self.rotary_cos_emb_txt, self.rotary_sin_emb_txt)
        return self._rotary_interleaved_torch(modality, sample_ids)

    def _rotary_interleaved_torch(self, modality, sample_ids):
        """models/dit.py:1421-1444 with `add_img_data_to_blocks` / `add_txt_data_to_blocks` (:122-191), as tensor operations on the device (the
        reference loops over blocks on the host): cos, sin fp32 [B, L, D/2] and, per position, the row of `img_count_embedding` to add (-1: none).
        Image runs whose length is a supported block size get that size's 2-D table and count embedding j = number of earlier image runs of the row
        that start in the same packed sample; text positions inside a run of one sample id >= 0 get the 1-D table from the start of that run;
        everything else (padding, image runs of other lengths) keeps cos = sin = 0."""
        B, L = modality.shape
        dev = modality.device
        ar = torch.arange(L, device=dev)[None].expand(B, L)
        is_img = modality.bool()
        prev = torch.nn.functional.pad(is_img[:, :-1], (1, 0))
        start = is_img & ~prev
        run_start = torch.cummax(torch.where(start, ar, torch.full_like(ar, -1)), dim=1).values
        rows = torch.arange(B, device=dev)[:, None].expand(B, L)
        key = (rows * L + run_start.clamp(min=0))
        # (static shapes only - no boolean-mask indexing, no host reads: the host must be able to run ahead of the device across this preamble)
        counts = torch.bincount(torch.where(is_img, key, torch.full_like(key, B * L)).reshape(-1), minlength=B * L + 1)[: B * L]
        run_len = torch.where(is_img, counts[key], torch.zeros_like(key))
        pos_in_run = ar - run_start
        if getattr(self, "_img_tab_cos", None) is None or self._img_tab_cos.device != dev:
            self._img_tab_cos = torch.cat([getattr(self, f"rotary_cos_emb_img_{n}") for n, _ in self.IMG_BLOCKS], 0).to(dev)
            self._img_tab_sin = torch.cat([getattr(self, f"rotary_sin_emb_img_{n}") for n, _ in self.IMG_BLOCKS], 0).to(dev)
        off = torch.full_like(run_len, -1)
        base = 0
        for n, _ in self.IMG_BLOCKS:
            off = torch.where(run_len == n, torch.full_like(off, base), off)
            base += n
        valid_img = is_img & (off >= 0)
        idx = (off + pos_in_run).clamp(min=0)
        cos_img, sin_img = self._img_tab_cos[idx], self._img_tab_sin[idx]
        # image index inside its packed sample: running count of image-run starts per (row, sample id)
        sid = sample_ids
        # rank of every image-run start among the starts of its (row, sample id), in position order: stable sort of the flattened positions by group key (non-starts
        # sort behind every group), rank = index in the sorted order - index of the group's first element.  No one-hot over the number of sample ids (which would need it
        # on the host), any layout of ids inside a row.
        N = B * L
        flat_start = start.reshape(-1)
        gkey = torch.where(flat_start, (rows * (L + 2) + sid.clamp(min=-1) + 1).reshape(-1), torch.full((N,), B * (L + 2) + 1, dtype=torch.int64, device=dev))
        order = torch.argsort(gkey, stable=True)
        skey = gkey[order]
        arn = torch.arange(N, device=dev)
        newg = torch.ones(N, dtype=torch.bool, device=dev)
        newg[1:] = skey[1:] != skey[:-1]
        g_first = torch.cummax(torch.where(newg, arn, torch.zeros_like(arn)), 0).values
        j_at = torch.empty(N, dtype=torch.int64, device=dev).scatter_(0, order, arn - g_first).reshape(B, L)   # valid at run starts (read only there)
        j_run = j_at.gather(1, run_start.clamp(min=0))
        count_idx = torch.where(valid_img, j_run, torch.full_like(j_run, -1))
        # text: positions restart at every run of one sample id
        sprev = torch.nn.functional.pad(sid[:, :-1], (1, 0), value=-2)
        sstart = sid != sprev
        s_run_start = torch.cummax(torch.where(sstart, ar, torch.full_like(ar, -1)), dim=1).values
        tpos = (ar - s_run_start).clamp(min=0, max=self.rotary_cos_emb_txt.shape[0] - 1)
        is_txt = (~is_img) & (sid >= 0)
        zero = torch.zeros((), dtype=cos_img.dtype, device=dev)
        cos = torch.where(valid_img[:, :, None], cos_img, torch.where(is_txt[:, :, None], self.rotary_cos_emb_txt[tpos], zero))
        sin = torch.where(valid_img[:, :, None], sin_img, torch.where(is_txt[:, :, None], self.rotary_sin_emb_txt[tpos], zero))
        return cos.contiguous(), sin.contiguous(), count_idx

    def _rotary(self, modality, L):
        """models/dit.py:1413-1460 (non-interleaved branches) → fp32 [L, D/2] or per-sample [B, L, D/2]."""
        if self.modality_embed is not None and self.rope_2d and self.multimodal_batches:
            ci, si = self.rotary_cos_emb_img, self.rotary_sin_emb_img
            if modality.shape[-1] != self.img_length:
                pad = max(modality.shape[-1] - self.img_length, 0)
                nanpad = torch.full((pad, ci.shape[-1]), float("nan"), device=ci.device, dtype=ci.dtype)
                ci, si = torch.cat([nanpad, ci], 0), torch.cat([nanpad, si], 0)
            sel = modality[:, :, None] == 0
            cos = torch.where(sel, self.rotary_cos_emb_txt[None, :L], ci[None, :L]).contiguous()
            sin = torch.where(sel, self.rotary_sin_emb_txt[None, :L], si[None, :L]).contiguous()
            return cos, sin
        return self.rotary_cos_emb[:L].contiguous(), self.rotary_sin_emb[:L].contiguous()

    def _engine_forward(self, inp: _EngineInputs, mode, save):
        """-> (by `mode`: "logits" [B, L, V] / "logp" log p(x0 | xt) [B, L] through the fused head / "rows" the sampler's [MASK]-row logits; the forward's _Saved)"""
        K.require_gpu(inp.indices)
        (B, L), dev = inp.indices.shape, inp.indices.device
        if (B * L) % 8 != 0:
            raise ValueError(f"unidisc_amd.DIT: batch*length = {B * L} must be a multiple of 8")
        S = _Saved(mode=mode, save=save, B=B, L=L, nt=K.norm_id(self.norm_type), kv_sink=inp.kv_sink, kv_read=inp.kv_read, ada_cache={}, blocks=[],
                   ckpt=bool(self.use_gradient_checkpointing) and save)
        self.refresh_weight_shadows(rows=B * L)
        S.p_drop = self.dropout if self.training else 0.0
        if self.training and save:   # only training forwards advance the dropout stream (eval / sampler passes draw no dropout masks)
            self._fwd_count += 1
        S.seed0 = ((torch.initial_seed() * 1000003 + self._fwd_count * 4096) ^ (self._dropout_rank() * 0x9E3779B97F4A7C15)) & ((1 << 62) - 1)
        S.ids = inp.indices.contiguous().view(-1).to(torch.int64)
        S.modality = inp.modality.contiguous().view(-1).to(torch.int64) if inp.modality is not None else None
        S.emb_mod = S.modality
        if self.modality_embed is not None and S.modality is None:
            if self.multimodal_batches:
                raise ValueError("unidisc_amd.DIT: modality_embed with multimodal_batches needs the `modality` argument")
            S.emb_mod = self._static_modality(B, L, dev).view(-1)   # static slices (models/dit.py:1409-1411)
        raw_sid = self._attention_masks(S, inp, dev)
        S.dgrad_form = {name: lin.dgrad_form() for name, lin in self._lins.items()}   # NN vs NT per Linear, fixed by THIS forward's shadows (not re-derived at backward time)
        ce = self._plan_head(S, inp, dev)
        x = K.embedding_fwd(S.ids, self.vocab_embed.embedding.detach(), S.emb_mod if self.modality_embed is not None else None,
                            self.modality_embed.embedding.detach() if self.modality_embed is not None else None)
        self._rotary_rows(S, inp, x, raw_sid)
        if self.time_conditioning:
            self._sigma_map_forward(S, inp.sigma, dev)
        pre = None
        for i in range(self.n_blocks):
            x, pre, R = self._block_forward(S, i, x, pre)
            S.blocks.append(R)   # (None unless `save`)
        self._await_cast("head")
        fmod = self._ada_mod(S, self.n_blocks) if self.time_conditioning else None   # [Bp, 2d]
        hf, rstdf, meanf = pre if pre is not None else K.norm_fwd(x, self.output_layer.norm_final.weight.detach(), S.nt, L, mod=fmod, mod_idx=(0, 1),
                                                                  modality=S.modality, any_img=S.any_img)
        S.ada_cache = S.ada_cache if S.ckpt else None   # (only the checkpointing recompute reads it again)
        if save:
            S.x_final, S.rstdf, S.meanf, S.fmod = x, rstdf, meanf, fmod
        if mode == "rows":
            return self._head_rows(S, hf), S
        if mode == "logits":
            return self._head_logits(S, hf, inp.head_out), S
        return self._head_logp(S, inp, hf, ce), S

    def _attention_masks(self, S, inp, dev):
        """Sample ids -> mask codes -> key mask -> doc_ranges: what the attention kernels take in their sample-id slot (S.sid, S.doc_ranges), the attention-dropout
        probability (S.p_attn), the combinations that are refused.  Returns the document ids as given (the per-sample rotary positions need them without class bits)."""
        sid = raw_sid = inp.sample_ids.contiguous().to(torch.int64) if inp.sample_ids is not None else None
        bm, km = inp.block_mask, inp.key_mask
        if self.causal and (sid is not None or isinstance(bm, ModalityMask) or km is not None):
            raise NotImplementedError("unidisc_amd.DIT: causal attention (model.full_attention=false) with packed sample_ids, a ModalityMask or an attention mask - "
                                      "the reference never combines is_causal with another mask")
        S.doc_ranges = K.attention_doc_ranges(sid) if sid is not None else None   # once per step, shared by every block's forward and backward
        if isinstance(bm, ModalityMask) and sid is None:
            # modality attention dropout (model.py:863-878): an asymmetric per-sample mask, carried to the attention kernels as mask codes in
            # the sample-id slot (class bits: no tile skipping, every tile takes the per-element test)
            sid = K.modality_mask_codes(bm.txt_drop.to(dev), bm.img_drop.to(dev), bm.txt_length, S.L)
        if km is not None:
            # key-padding mask (model.use_attention_mask): padded keys get a key class (4) no query mask contains; positions without other codes become
            # sample 0 / key class 1 / query mask "classes 1 | 2".  Class bits switch tile skipping off (doc_ranges = None): every tile takes the element test.
            km = km.to(dev).reshape(S.B, S.L)
            base = sid if sid is not None else torch.zeros((S.B, S.L), dtype=torch.int64, device=dev)
            kbits, qbits = (base >> 32) & 0xff, (base >> 40) & 0xff
            kbits = torch.where(km, torch.where(kbits == 0, torch.ones_like(kbits), kbits), torch.full_like(kbits, 4))
            qbits = torch.where(qbits == 0, torch.full_like(qbits, 3), qbits)
            sid = ((base & 0xffffffff) | (kbits << 32) | (qbits << 40)).contiguous()
            S.doc_ranges = None
        S.sid = sid
        S.p_attn = self.attn_dropout if self.training else 0.0
        if S.p_attn > 0.0 and sid is not None:
            raise NotImplementedError("unidisc_amd.DIT: model.attn_dropout with packed sample_ids, a ModalityMask or an attention mask - the reference's "
                                      "FlexAttention path applies no attention dropout")
        # (a causal backbone reads a cache only through the causal kernel: _KVRead.causal, the chunked cached forward)
        if S.kv_read is not None and (sid is not None or S.save or S.kv_sink is not None or self.causal != bool(S.kv_read.causal) or
                                      (S.kv_read.causal and (S.kv_read.split or self.time_conditioning))):
            raise NotImplementedError("unidisc_amd.DIT: the cache-reading forward is an inference path without masks (no sample ids, ModalityMask, attention mask)")
        return raw_sid

    def _plan_head(self, S, inp, dev):
        """SUBS: only [MASK] rows have a non-zero log-probability (model.py:621-658), so in "logp" mode the vocabulary head (GEMM fwd, dgrad, wgrad and the
        cross-entropy) runs on the masked rows only.  Their number is data dependent: it is counted on a side stream NOW (S.head_plan) and only read back right
        before the head, when the host has already queued every block of this forward - the device never waits for the host.  Returns the operands of the AR
        baseline's shifted head (ar_head_operands: row r predicts token r + 1), or None."""
        B, L, mode, restrict, ce = S.B, S.L, S.mode, bool(inp.restrict), None
        if mode == "logp" and bool(inp.ar_shift):
            ar_mod = inp.modality.reshape(B, L) if inp.modality is not None else (self._static_modality(B, L, dev) if restrict else None)
            ce = ar_head_operands(inp.x0.reshape(B, L), ar_mod, self.mask_index)
        split_ok = (mode == "logp" and self.compact_head and self.split_head and restrict and S.modality is not None and inp.plan_ids is None
                    and 0 < self.text_vocab_size < self.vocab_size and self.head_chunk_rows <= 0)
        plan_src, plan_mod = (ce[0], ce[2]) if ce is not None else (S.ids if inp.plan_ids is None else inp.plan_ids.reshape(S.ids.shape), S.modality)
        if (mode == "logp" and self.compact_head) or mode == "rows":
            S.head_plan = self._plan_masked_rows(plan_src, plan_mod if split_ok else None)
        return ce

    def _rotary_rows(self, S, inp, x, raw_sid):
        """The rotary tables of this forward's rows (S.cos, S.sin); packed batches also add the image-count embedding to x."""
        if self.rope_2d and self.require_sample_ids:
            if raw_sid is None:
                raise ValueError("unidisc_amd.DIT: data.require_sample_ids needs sample_ids")
            S.cos, S.sin, count_idx = self._rotary_interleaved(inp.modality.to(torch.int64), raw_sid)
            # x[b, l] += img_count_embedding[j] on the positions of supported image blocks.  Static shapes (no nonzero(): that is a host read in the step's preamble):
            # every position gathers a row of the table extended by one zero row, positions without an image index take that row
            n_cnt = self.img_count_embedding.shape[0]
            S.cnt_j = torch.where(count_idx.view(-1) >= 0, count_idx.view(-1), torch.full_like(count_idx.view(-1), n_cnt))
            tab = torch.cat([self.img_count_embedding.detach().to(x.dtype), torch.zeros((1, x.shape[1]), dtype=x.dtype, device=x.device)], 0)
            x.add_(tab.index_select(0, S.cnt_j))
        elif inp.rope is not None:   # (the cached paths: rows of the full-length tables)
            S.cos, S.sin = inp.rope
        else:
            S.cos, S.sin = self._rotary(inp.modality, S.L)

    def _sigma_map_forward(self, S, sigma, dev):
        """c = silu(W2 silu(W0 te + b0) + b2), the conditioning every adaLN_modulation reads"""
        if sigma is None:
            raise ValueError("unidisc_amd.DIT: time_conditioning needs sigma")
        lin, sigma = self._lins, sigma.reshape(-1).to(F32).contiguous()
        S.Bp = _ceil(S.B, 8)
        S.te = torch.zeros((S.Bp, 256), dtype=BF16, device=dev)
        K.timestep_embedding(sigma, S.te, S.B, 256)
        self._await_cast("pre")
        S.l1 = K.gemm_nt(S.te, lin["sig0"].w16, N=lin["sig0"].out, epilogue=K.EPI_BIAS, bias=lin["sig0"].bias.detach())
        S.s1 = K.silu_fwd(S.l1)
        S.l2 = K.gemm_nt(S.s1, lin["sig2"].w16, N=lin["sig2"].out, epilogue=K.EPI_BIAS, bias=lin["sig2"].bias.detach())
        S.c = K.silu_fwd(S.l2)
        if S.modality is not None:
            S.any_img = (S.modality != 0).any().to(torch.int32).reshape(1)

    def _ada_mod(self, S, i):
        """adaLN_modulation(c) of block i (i == n_blocks: the final layer's), computed once per forward: the residual add in front of a modulated norm needs it
        one block early"""
        key = str(i) if i < self.n_blocks else "head"
        if key not in S.ada_cache:
            self._await_cast(i if i < self.n_blocks else "head")
            a = self._lins[f"{key}.ada"]
            S.ada_cache[key] = K.gemm_nt(S.c, a.w16, N=a.out, epilogue=K.EPI_BIAS, bias=a.bias.detach())   # [Bp, 6d] (final layer: [Bp, 2d]) bf16
        return S.ada_cache[key]

    def _block_forward(self, S, i, x, pre, last_rows=None, recompute=False):
        """One DiT block: x [M, d] fp32 -> (x_out, pre_out, what the block's backward reads).  `recompute` (activation checkpointing, models/dit.py:1486-1490): the
        backward re-runs the block from its saved input - same kernels, same dropout seeds, the fused next-block pre-norm replaced by the block's own norm kernel
        (bit-identical) - so only x_in (and the compacted row list of the last block) is kept per block."""
        blk, lin, tc, sw = self.blocks[i], self._lins, self.time_conditioning, self.sandwich_normalization
        B, L, nt, mod_flat, any_img, p_drop, seed0 = S.B, S.L, S.nt, S.modality, S.any_img, S.p_drop, S.seed0
        M, d, H, D = B * L, self.hidden_size, self.n_heads, self.head_dim
        if not recompute:
            self._await_cast(i)
        mod = self._ada_mod(S, i) if tc else None   # [Bp, 6d] bf16
        # (norm1 comes fused out of the previous block's MLP residual add where there is one)
        h1, rstd1, mean1 = pre if pre is not None else K.norm_fwd(x, blk.norm1.weight.detach(), nt, L, mod=mod, mod_idx=(0, 1), modality=mod_flat, any_img=any_img)
        qkv = K.gemm_nt(h1, lin[f"{i}.qkv"].w16, N=3 * d)
        at, qn = blk.attention, self.qk_norm
        qkr, qstats = K.qknorm_rope_fwd(qkv, S.cos, S.sin, L, D, q_scale=self.attn_q_scale, gq=at.q_norm.weight.detach() if qn else None,
                                        bq=at.q_norm.bias.detach() if qn else None, gk=at.k_norm.weight.detach() if qn else None,
                                        bk=at.k_norm.bias.detach() if qn else None)
        if S.kv_sink is not None:   # KV-cache prefill: the post-rope k and the v of every position into cache slots [0, L)
            S.kv_sink[i][0][:, :L].copy_(qkr.view(B, L, 2 * d)[:, :, d:])
            S.kv_sink[i][1][:, :L].copy_(qkv.view(B, L, 3 * d)[:, :, 2 * d:])
        kvr = S.kv_read
        if kvr is not None:   # this call's post-rope k and v into cache slots [slot0, slot0 + L) (the kernel only reads), then the L queries against slots [0, Lk)
            s0 = kvr.slot0
            kvr.K[i][:, s0:s0 + L].copy_(qkr.view(B, L, 2 * d)[:, :, d:])
            kvr.V[i][:, s0:s0 + L].copy_(qkv.view(B, L, 3 * d)[:, :, 2 * d:])
            if kvr.causal:
                o, lse = K.attention_fwd_kv_causal(qkr[:, :d], kvr.K[i], kvr.V[i], B, L, kvr.Lk, H, D, q_prescaled=True), None
            elif kvr.split:
                o, lse = K.attention_fwd_kv_split(qkr[:, :d], kvr.K[i], kvr.V[i], B, L, kvr.Lk, H, D, q_prescaled=True, ws=kvr.ws), None
            else:
                o, lse = K.attention_fwd_kv(qkr[:, :d], kvr.K[i], kvr.V[i], B, L, kvr.Lk, H, D, q_prescaled=True), None
        else:
            o, lse = K.attention_fwd(qkr, qkv, B, L, H, D, S.sid, S.doc_ranges, q_prescaled=True, **self._attn_mask_kw, **S.attn_drop_kw(i))
        rows_c = last_rows   # (None unless `recompute`)
        if not recompute and i + 1 == self.n_blocks and S.head_plan is not None and S.mode == "logp" and self.compact_last_block and not tc:
            head_rows_c = self._masked_rows(S.head_plan, M)   # (the count was queued at the top of this forward: the host does not wait for the device here)
            rows_c = head_rows_c[0] if head_rows_c is not None else None
        x_full, o_full = x, o
        if rows_c is not None:   # from here on this block works on the [MASK] rows (+ padding) only
            o = o.index_select(0, rows_c)
            x = x.index_select(0, rows_c)
        a_out = K.gemm_nt(o, lin[f"{i}.out"].w16, N=d)
        # The next pre-norm is fused into the residual add (x_out is normalised while in registers) - with adaLN in its modulated form (round 5)
        fuse_w2 = blk.norm2.weight.detach()
        nkw2 = dict(next_mod=mod, next_mod_idx=(3, 4), next_modality=mod_flat, next_any_img=any_img) if tc else {}
        if sw:  # x = x_skip + pre_residual_norm(attn)   (dit.py:993-994; no gate, no dropout)
            res = K.residual_fwd(x, a_out, L, w_b=blk.pre_residual_norm.weight.detach(), norm_type=nt, next_w=fuse_w2, **nkw2)
        else:   # bias_dropout_add_scale with gate_msa on every token (Attention.time_conditioning is never set: dit.py:533,884)
            res = K.residual_fwd(x, a_out, L, norm_type=nt, mod=mod, gate_idx=2 if tc else None, p_drop=p_drop, seed=seed0 + 4 * i + 1, next_w=fuse_w2, **nkw2)
        x_mid, rstd_a, mean_a, (h2, rstd2, mean2) = res[:4]
        f1, f2 = lin[f"{i}.fc1"], lin[f"{i}.fc2"]
        u1 = torch.empty((o.shape[0], 4 * d), dtype=BF16, device=x.device)
        g = K.gemm_nt(h2, f1.w16, N=4 * d, epilogue=K.EPI_BIAS_GELU, bias=f1.bias.detach(), aux=u1)
        u2 = K.gemm_nt(g, f2.w16, N=d, epilogue=K.EPI_BIAS, bias=f2.bias.detach())
        # the consumer of x_out: norm1 of the next block, or norm_final (with adaLN: modulated by the NEXT block's / the final layer's adaLN output)
        nxt_w = (self.blocks[i + 1].norm1.weight if i + 1 < self.n_blocks else self.output_layer.norm_final.weight).detach()
        nkw = dict(next_mod=self._ada_mod(S, i + 1), next_mod_idx=(0, 1), next_modality=mod_flat, next_any_img=any_img) if tc and not recompute else {}
        if tc and recompute:      # (recomputation of ONE block in the backward: its output's norm is not needed)
            nxt_w = None
        res = K.residual_fwd(x_mid, u2, L, w_b=blk.post_ff_norm.weight.detach() if sw else None, norm_type=nt, mod=mod,
                             gate_idx=5 if tc else None, modality=mod_flat if tc else None, p_drop=p_drop, seed=seed0 + 4 * i + 2, next_w=nxt_w, **nkw)
        x_out, rstd_m, mean_m = res[:3]
        pre = res[3] if nxt_w is not None else None
        R = None
        if S.save and S.ckpt and not recompute:
            R = _BlockActs(ckpt=True, x_in=x_full, rows_c=rows_c)
        elif S.save:
            R = _BlockActs(mod=mod, x_in=x_full, h1=h1, rstd1=rstd1, mean1=mean1, qkv=qkv, qkr=qkr, qstats=qstats, o=o_full, lse=lse, a_out=a_out, rstd_a=rstd_a,
                           mean_a=mean_a, x_mid=x_mid, h2=h2, rstd2=rstd2, mean2=mean2, u1=u1, g=g, u2=u2, rstd_m=rstd_m, mean_m=mean_m, rows_c=rows_c,
                           o_c=o if rows_c is not None else None)
        return x_out, pre, R

    def _head_split_cols(self):
        """Split head: (text rows) x ids [0, c_up) + (image rows) x ids [c_al, V).  The boundary is rounded to multiples of 8 outwards so that every operand and
        output pointer keeps its alignment; the few extra columns are never read (the cross-entropy reads a row's valid ids only)."""
        return self.text_vocab_size // 8 * 8, _ceil(self.text_vocab_size, 8)

    def _head_gemm(self, rows, out, c0=0, c1=None):
        """out = rows W[c0:c1]^T + b[c0:c1]: the vocabulary head (c1 = None: up to V), or a column range of it"""
        head = self._lins["head"]
        return K.gemm_nt(rows, head.w16[c0:], out=out, N=(self.vocab_size if c1 is None else c1) - c0, epilogue=K.EPI_BIAS, bias=head.bias.detach()[c0:])

    def _head_rows(self, S, hf):
        """sampler: logits of the [MASK] rows only (no autograd); rows = their flat indices, padded to a multiple of 64"""
        rows_p, n_masked = self._masked_rows(S.head_plan, S.B * S.L, always=True)
        logits = torch.empty((rows_p.numel(), self._lins["head"].outp), dtype=BF16, device=hf.device)
        self._head_gemm(hf.index_select(0, rows_p), logits)
        return logits, rows_p, n_masked

    def _head_logits(self, S, hf, head_out):
        B, L, V = S.B, S.L, self.vocab_size
        if head_out is not None:   # (KV-cache prefill: the head on each row's last position only)
            last = torch.arange(B, device=hf.device) * L + (L - 1)
            self._head_gemm(hf.index_select(0, last), head_out)
            return head_out
        logits = torch.empty((B * L, self._lins["head"].outp), dtype=BF16, device=hf.device)
        self._head_gemm(hf, logits)
        if S.save:
            S.hf, S.logits = hf, logits
        return logits[:, :V].view(B, L, V)

    def _head_logp(self, S, inp, hf, ce):
        """The fused head + SUBS cross-entropy: log p(x0 | xt) [B, L] fp32, on the [MASK] rows only where the plan compacts them."""
        B, L, M, dev, restrict = S.B, S.L, S.B * S.L, hf.device, bool(inp.restrict)
        ids_h, x0, ce_mod = ce if ce is not None else (S.ids, inp.x0, S.modality)
        if ce is None and restrict and S.modality is None:  # static slices (model.py:634-635)
            ce_mod = self._static_modality(B, L, dev).view(-1)
        x0 = x0.contiguous().view(-1).to(torch.int64)
        head_rows = self._masked_rows(S.head_plan, M) if S.head_plan is not None else None
        stream_compact = head_rows is not None and hf.shape[0] != M   # the last block already runs on the compacted rows (same list, same order)
        hf_h = hf
        if head_rows is not None:  # compact operands: masked rows first, padded (with an unmasked row: zero loss, zero gradient) to a multiple of 64
            rows_p = head_rows[0]
            # fixed-capacity buffers (views of M-row allocations): a different size every step would make the caching allocator go back
            # to hipMalloc until its pool covers every size seen (measured: occasional 120+ ms steps)
            hf_h = hf if stream_compact else torch.index_select(hf, 0, rows_p, out=torch.empty_like(hf)[: rows_p.numel()])
            x0, ids_h = x0.index_select(0, rows_p), ids_h.index_select(0, rows_p)
            ce_mod = ce_mod.index_select(0, rows_p) if ce_mod is not None else None
        chunk = _ceil(self.head_chunk_rows, 64) if self.head_chunk_rows > 0 else 0
        chunk = chunk if chunk < hf_h.shape[0] else 0
        groups = S.head_plan.get("groups") if (S.head_plan is not None and head_rows is not None and restrict and not chunk) else None
        ce_args = (self.vocab_size, self.text_vocab_size, self.mask_index, restrict)
        if chunk:   # fused head + cross-entropy over row chunks: only one chunk of logits exists at a time, none is kept
            logits, buf, parts = None, torch.empty((chunk, self._lins["head"].outp), dtype=BF16, device=dev), []
            for r0 in range(0, hf_h.shape[0], chunk):
                r1 = min(hf_h.shape[0], r0 + chunk)
                self._head_gemm(hf_h[r0:r1], buf[: r1 - r0])
                parts.append(K.subs_ce_fwd(buf[: r1 - r0], x0[r0:r1], ids_h[r0:r1], ce_mod[r0:r1] if ce_mod is not None else None, *ce_args))
            log_p, lse_ce = (torch.cat(t) for t in zip(*parts))
        else:
            logits = torch.empty((M, self._lins["head"].outp), dtype=BF16, device=dev)[:hf_h.shape[0]]
            if groups is not None:
                (n_tp, n_ip), (c_al, c_up) = groups, self._head_split_cols()
                if n_tp:
                    self._head_gemm(hf_h[:n_tp], logits[:n_tp], 0, c_up)
                if n_ip:
                    self._head_gemm(hf_h[n_tp:], logits[n_tp:, c_al:], c_al)
            else:
                self._head_gemm(hf_h, logits)
            log_p, lse_ce = K.subs_ce_fwd(logits, x0, ids_h, ce_mod, *ce_args)
        if head_rows is not None:   # (padding rows are unmasked: their log p is exactly 0, like every row left out)
            log_p = torch.zeros(M, dtype=log_p.dtype, device=dev).index_copy_(0, rows_p, log_p)
        if S.save:
            S.hf, S.logits, S.head_rows, S.ids_h, S.x0, S.ce_mod, S.restrict, S.lse_ce = hf_h, logits, head_rows, ids_h, x0, ce_mod, restrict, lse_ce
            S.stream_compact, S.head_chunk, S.head_groups = stream_compact, chunk, groups
        return log_p.view(B, L)

    def _static_modality(self, B, L, dev):
        return static_modality(B, L, self.static_img_sl, dev)

    def _plan_masked_rows(self, ids, mod=None):
        """Queue (without synchronising) a stable partition of the row indices with the [MASK] rows first and their count.  With `mod` (the rows' modality,
        0 = text / 1 = image) the [MASK] rows are ordered text first, then image, and both counts are reported: the vocabulary head can then run as two
        (rows of one modality) x (ids valid for that modality) problems (`_masked_rows`, split_head)."""
        is_mask = ids == self.mask_index
        if mod is not None:
            key = (~is_mask).to(torch.int8) * 2 + (mod == 1).to(torch.int8)     # 0 masked text, 1 masked image, 2 / 3 unmasked
            counts = lambda: torch.stack([(is_mask & (mod != 1)).sum(), (is_mask & (mod == 1)).sum()])
        else:
            key = (~is_mask).to(torch.int8)
            counts = lambda: is_mask.sum().view(1)
        if not ids.is_cuda:  # CPU orchestration tests
            c = counts()
            return dict(order=torch.argsort(key, stable=True), count=int(c.sum()), count2=(int(c[0]), int(c[1])) if mod is not None else None, event=None)
        dev = ids.device
        main = torch.cuda.current_stream(dev)
        side = self._side_streams.get(dev) if getattr(self, "_side_streams", None) else None
        if side is None:   # one side stream per device the module has run on
            self._side_streams = dict(getattr(self, "_side_streams", None) or {})
            side = self._side_streams[dev] = torch.cuda.Stream(device=dev)
        count_host = torch.empty(2 if mod is not None else 1, dtype=torch.int64).pin_memory()   # per call: forwards on two streams / threads must not share the counter
        side.wait_stream(main)
        with torch.cuda.stream(side):
            order = torch.argsort(key, stable=True)
            count_host.copy_(counts(), non_blocking=True)
            event = torch.cuda.Event()
            event.record(side)
        is_mask.record_stream(side)
        key.record_stream(side)
        order.record_stream(main)
        return dict(order=order, count=None, count2=None, event=event, count_host=count_host, side=side, by_modality=mod is not None)

    def _masked_rows(self, plan, M, always=False):
        """(row indices: the [MASK] rows, then as many unmasked rows as pad the list to a multiple of 64; number of masked rows), or
        None when compaction would not shrink the head.  Unmasked rows have zero loss and zero gradient, so padding with them is exact."""
        if plan.get("n") is not None:
            n = plan["n"]
        elif plan["event"] is not None:
            plan["event"].synchronize()
            ch = plan["count_host"]
            if plan.get("by_modality"):
                plan["count2"] = (int(ch[0]), int(ch[1]))
            n = int(ch.sum())
            torch.cuda.current_stream().wait_stream(plan["side"])
        else:
            n = plan["count"]
        plan["n"] = n
        if "rows" in plan:       # (decided once per forward: the last block's compaction and the head must see the same list)
            return plan["rows"]
        plan["groups"] = None
        n_pad = _ceil(max(n, 1), 64)
        if n_pad >= M:
            plan["rows"] = (plan["order"], n) if always else None   # always: every row, [MASK] rows first
            return plan["rows"]
        c2 = plan.get("count2")
        if c2 is not None and not always and self.split_head and n > 0:
            # two groups - [MASK] text rows, [MASK] image rows - each padded to a multiple of 64 with unmasked rows (zero loss, zero gradient: exact)
            n_t, n_i = c2
            n_tp, n_ip = (_ceil(n_t, 64) if n_t else 0), (_ceil(n_i, 64) if n_i else 0)
            pad_t, pad_i = n_tp - n_t, n_ip - n_i
            if n_tp + n_ip < M and pad_t + pad_i <= M - n:
                o = plan["order"]
                plan["rows"] = (torch.cat([o[:n_t], o[n:n + pad_t], o[n_t:n], o[n + pad_t:n + pad_t + pad_i]]), n)
                plan["groups"] = (n_tp, n_ip)
                return plan["rows"]
        plan["rows"] = (plan["order"][:n_pad], n)
        return plan["rows"]

    # -------------------------------------------------------------------------------------------- engine: backward
    def _alloc_grads(self, params, dev):
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += _ceil(p.numel(), 64)
        # GEMM weights (92 % of the buffer) are fully overwritten by their wgrad kernel; only atomically accumulated gradients
        # (norm / bias / qk-norm vectors, embeddings) and the alignment gaps need zeroing.
        flat = torch.empty(total, dtype=F32, device=dev)
        gemm_w = {id(l.weight) for l in self._lins.values()}
        lo, gaps = None, []
        for p, o in zip(params, offs):
            end = o + _ceil(p.numel(), 64)
            if id(p) in gemm_w:
                if lo is not None:
                    gaps.append(flat[lo:o])
                    lo = None
                if end > o + p.numel():
                    gaps.append(flat[o + p.numel():end])
            elif lo is None:
                lo = o
        if lo is not None:
            gaps.append(flat[lo:total])
        if gaps:   # ~70 short ranges: one multi-tensor launch instead of one fill kernel each
            torch._foreach_zero_(gaps)
        self._grad_ranges = {id(p): (o, o + _ceil(p.numel(), 64)) for p, o in zip(params, offs)}
        return flat, {id(p): flat[o:o + p.numel()].view(p.shape) for p, o in zip(params, offs)}

    def _notify(self, flat, group):
        """Tell the gradient-sync hook that the flat range covering `group` (contiguous by construction) is final."""
        cb = self.grad_ready_callback
        if cb is None or not group:
            return
        lo = min(self._grad_ranges[id(p)][0] for p in group)
        hi = max(self._grad_ranges[id(p)][1] for p in group)
        cb(flat, lo, hi)

    def _wgrad(self, dY, X, lin: _Lin, G, n_rows=None, bias_done=False, beta=0.0):
        """dW[out,in] = dY[M,out]^T X[M,in] (fp32), db = colsum(dY).  dY/X bf16 [M, *]."""
        (Mrows, outp), db = dY.shape, None
        if lin.bias is not None and not bias_done:
            db = G[id(lin.bias)] if outp == lin.out else torch.zeros(outp, dtype=F32, device=dY.device)
        few_tiles = K.gemm_tn_wants_splitk(lin.out, lin.inp)
        if Mrows % 64 == 0:  # K-major GEMM reads dY and X in place (transposing LDS reads); bias grad = column sums
            if db is not None:
                K.colsum(dY, db)
            if few_tiles:  # e.g. the 2048 x 2048 out-proj weight: 64 tiles over K = B*L -> split K through a workspace
                K.gemm_tn_splitk(dY, X, G[id(lin.weight)], M=lin.out, N=lin.inp, beta=beta)
            else:
                K.gemm_tn(dY, X, G[id(lin.weight)], M=lin.out, N=lin.inp, beta=beta)
        else:  # short contraction (e.g. adaLN over the padded batch): explicit transposes + NT kernel
            dYt = K.transpose(dY, colsum=db)
            Xt = K.transpose(X)
            K.gemm_nt(dYt, Xt, out=G[id(lin.weight)], M=lin.out, N=lin.inp, K=Mrows, beta=beta)
        if db is not None and outp != lin.out:
            if beta != 0.0:
                G[id(lin.bias)].add_(db[: lin.out])
            else:
                G[id(lin.bias)].copy_(db[: lin.out])

    def _engine_backward(self, S: _Saved, grad_out, mode):
        params = self._ordered_params()
        M, d, dev = S.B * S.L, self.hidden_size, S.ids.device
        bp = _Backward(S=S, nt=K.norm_id(self.norm_type), ada_off=0)
        bp.flat, bp.G = self._alloc_grads(params, dev)
        G, tc, fl = bp.G, self.time_conditioning, self.output_layer
        dhf = self._head_backward(bp, grad_out, mode)
        dmodf = None
        if tc:
            bp.dc = torch.zeros((S.Bp, self.cond_dim), dtype=F32, device=dev)
            dmodf = torch.zeros((S.Bp, 2 * d), dtype=F32, device=dev)
            # the adaLN_modulation backwards leave their input gradients as partial tiles in one buffer; summed once, where dc is consumed (`_sigma_map_backward`)
            if S.Bp <= K.SMALL_BATCH_LINEAR_MAX_B and self.cond_dim <= K.SMALL_BATCH_LINEAR_MAX_IN and self.cond_dim % 8 == 0:
                tiles = K.small_batch_linear_bwd_tiles(2 * d) + self.n_blocks * K.small_batch_linear_bwd_tiles(6 * d)
                bp.ada_buf = torch.empty((tiles, S.Bp, self.cond_dim), dtype=F32, device=dev)
        # (compacted last block: its residual-stream gradient lives on the compacted rows until the block's attention is reached)
        bp.dx = torch.empty((dhf.shape[0] if S.stream_compact else M, d), dtype=F32, device=dev)
        # (the final norm and each block's norm1 wait in `bp.pend` for the MLP branch below them, see _PendingNorm; with adaLN where the fused pass covers the shape)
        bp.tc_fused = tc and not S.stream_compact and K.norm_residual_bwd_ada_ok(M, d, S.L)
        pn = _PendingNorm(dy=dhf, x=S.x_final, rstd=S.rstdf, mean=S.meanf, w=fl.norm_final.weight.detach(), dw=G[id(fl.norm_final.weight)], accumulate=False,
                          mod=S.fmod, dmod=dmodf, mod_idx=(0, 1), finish=self.n_blocks)
        if tc:
            self._norm_backward(bp, pn)
        else:
            bp.pend = pn
        for i in reversed(range(self.n_blocks)):
            self._block_backward(bp, i)
        if bp.pend is not None:   # block 0's norm1 (or the final norm of a model without blocks): nothing below it to pair with
            self._norm_backward(bp, bp.pend)
        # ---- embeddings
        dx = bp.dx
        if S.cnt_j is not None:
            n_cnt = self.img_count_embedding.shape[0]
            if dx.is_cuda and dx.dtype == F32:   # sums formed in LDS per run of equal indices (an index_add_ here is 19 M contended atomics: 225 us)
                K.rowgroup_sum(dx, S.cnt_j, G[id(self.img_count_embedding)])
            else:
                gext = torch.zeros((n_cnt + 1, dx.shape[1]), dtype=dx.dtype, device=dx.device).index_add_(0, S.cnt_j, dx)   # (row n_cnt collects the positions without an image index)
                G[id(self.img_count_embedding)].add_(gext[:n_cnt])
        K.embedding_bwd(S.ids, dx, G[id(self.vocab_embed.embedding)], self.mask_index, modality=S.emb_mod if self.modality_embed is not None else None,
                        dEm=G[id(self.modality_embed.embedding)] if self.modality_embed is not None else None)
        tail = list(self.vocab_embed.parameters()) + (list(self.modality_embed.parameters()) if self.modality_embed is not None else [])
        if getattr(self, "img_count_embedding", None) is not None:
            tail.append(self.img_count_embedding)
        if tc:
            self._sigma_map_backward(bp)
            tail += list(self.sigma_map.parameters())
        self._notify(bp.flat, tail)
        if self.grad_sync_finish is not None:
            self.grad_sync_finish()
        # for the fused optimizer's one-pass global norm; a weak reference: the buffer lives exactly as long as the p.grad views do
        self._last_grad_flat_ref, self._last_grad_numel = weakref.ref(bp.flat), sum(p.numel() for p in params)
        return [G[id(p)] for p in params]

    def _head_backward(self, bp, grad_out, mode):
        """d logits -> dhf (the gradient of the final norm's output, on the rows the head ran on or scattered back to all rows), dW_head, db_head"""
        S, G, head = bp.S, bp.G, self._lins["head"]
        M, d, V, dev = S.B * S.L, self.hidden_size, self.vocab_size, S.ids.device
        logits, head_rows, groups = S.logits, S.head_rows, S.head_groups if mode == "logp" else None
        ce_args = (V, self.text_vocab_size, self.mask_index, S.restrict)
        if mode == "logp":
            g = grad_out.contiguous().view(-1).to(F32)
            if head_rows is not None:
                g = g.index_select(0, head_rows[0])
        if mode == "logp" and S.head_chunk:   # fused head + cross-entropy: per row chunk recompute the logits, form d logits in place, consume them (dgrad, wgrad accumulated)
            hf_h, chunk, cm, Mh = S.hf, S.head_chunk, S.ce_mod, S.hf.shape[0]
            dhf = torch.empty((M, d), dtype=BF16, device=dev)[:Mh]
            buf = torch.empty((chunk, head.outp), dtype=BF16, device=dev)
            for r0 in range(0, Mh, chunk):
                r1 = min(Mh, r0 + chunk)
                lg = buf[: r1 - r0]
                self._head_gemm(hf_h[r0:r1], lg)
                K.subs_ce_bwd(lg, S.x0[r0:r1], S.ids_h[r0:r1], cm[r0:r1] if cm is not None else None, S.lse_ce[r0:r1], g[r0:r1], *ce_args)
                K.gemm_nt_splitk(lg, head.w16t, N=d, out=dhf[r0:r1])
                self._wgrad(lg, hf_h[r0:r1], head, G, beta=0.0 if r0 == 0 else 1.0)
        else:
            if mode == "logp":
                K.subs_ce_bwd(logits, S.x0, S.ids_h, S.ce_mod, S.lse_ce, g, *ce_args, narrow_txt_rows=groups[0] if groups is not None else -1)
                dlogits = logits
            else:
                dlogits = torch.zeros_like(logits)
                dlogits[:, :V].copy_(grad_out.reshape(M, V))
            if groups is not None:   # the same two (rows of one modality) x (ids of that modality) problems as the forward; d logits is zero everywhere else
                (n_tp, n_ip), (c_al, c_up) = groups, self._head_split_cols()
                Vp, hf_h, Gw = head.outp, S.hf, G[id(head.weight)]
                k_t = min(_ceil(self.text_vocab_size, 64), Vp)
                dhf = torch.empty((M, d), dtype=BF16, device=dev)[: dlogits.shape[0]]
                db = torch.zeros(Vp, dtype=F32, device=dev)   # (column sums over widths that are multiples of 8; d logits is zero in the padding columns)
                if n_tp:
                    K.gemm_nt_splitk(dlogits[:n_tp, :k_t], head.w16t[:, :k_t], N=d, out=dhf[:n_tp])
                    K.colsum(dlogits[:n_tp, :c_up], db[:c_up])
                    if c_al:
                        K.gemm_tn(dlogits[:n_tp, :c_al], hf_h[:n_tp], Gw[:c_al], M=c_al, N=d)
                elif c_al:
                    Gw[:c_al].zero_()
                if n_ip:
                    K.gemm_nt_splitk(dlogits[n_tp:, c_al:], head.w16t[:, c_al:], N=d, out=dhf[n_tp:])
                    K.colsum(dlogits[n_tp:, c_al:], db[c_al:])
                    K.gemm_tn(dlogits[n_tp:, c_up:V], hf_h[n_tp:], Gw[c_up:], M=V - c_up, N=d)
                else:
                    Gw[c_up:].zero_()
                if c_up > c_al:   # the ids between the two aligned boundaries (at most 15) take every row
                    K.gemm_tn(dlogits[:, c_al:c_up], hf_h, Gw[c_al:c_up], M=c_up - c_al, N=d)
                G[id(head.bias)].copy_(db[:V])
            else:
                # few output tiles (compacted rows x d) over K = V: split K so that all CUs work (falls back to the plain kernel otherwise)
                dhf = K.gemm_nt_splitk(dlogits, head.w16t, N=d, out=torch.empty((M, d), dtype=BF16, device=dev)[: dlogits.shape[0]])
                self._wgrad(dlogits, S.hf, head, G)
        if head_rows is not None and not S.stream_compact:  # scatter the masked rows' gradient back; every other row of d(final norm output) is exactly zero
            dhf = torch.zeros((M, d), dtype=dhf.dtype, device=dev).index_copy_(0, head_rows[0], dhf)   # (padding rows: d logits = 0, so their rows of dhf are 0 too)
        S.logits = None
        return dhf

    def _finish_block(self, bp, i, dmod=None):
        """Block i (n_blocks: the final layer; None: nothing) has all its gradients but, with adaLN, those of its adaLN_modulation, which needs the shift / scale /
        gate gradients `dmod` collected up to here: run that backward, drop the block's activations, report its gradient range."""
        if i is None:
            return
        if dmod is not None:
            self._ada_backward(bp, dmod, self._lins[f"{i}.ada" if i < self.n_blocks else "head.ada"])
        if i < self.n_blocks:
            bp.S.blocks[i] = None
        self._notify(bp.flat, list((self.blocks[i] if i < self.n_blocks else self.output_layer).parameters()))

    def _norm_backward(self, bp, pn):
        """A pre-norm backward on its own: nothing below it to pair with, or (adaLN) a shape the fused pass does not cover."""
        S, ada = bp.S, pn.mod is not None
        K.norm_bwd(pn.dy, pn.x, pn.rstd, pn.mean, pn.w, bp.nt, S.L, bp.dx, pn.dw, accumulate=pn.accumulate, mod=pn.mod, dmod=pn.dmod, mod_idx=pn.mod_idx,
                   modality=S.modality if ada else None, any_img=S.any_img if ada else None)
        self._finish_block(bp, pn.finish, pn.dmod)

    def _norm_branch_bwd(self, bp, pn, branch, **kw):
        """Norm backward (`pn`, or None), then the backward of the residual branch below it on the dx it has just updated -> the branch's gradient: one fused pass
        where a kernel covers the pair, the two kernels otherwise.  `kw`: the branch's keywords of K.residual_bwd, and dbias (+= column sums of the result)."""
        S, dx, nt = bp.S, bp.dx, bp.nt
        if pn is not None and pn.mod is not None and not bp.tc_fused:
            self._norm_backward(bp, pn)
            pn = None
        if pn is None:
            dbias = kw.pop("dbias", None)
            out = K.residual_bwd(dx, branch, S.L, **kw)
            if dbias is not None:
                K.colsum(out, dbias)
            return out
        common = dict(accumulate=pn.accumulate, w_b=kw.get("w_b"), rstd_b=kw.get("rstd"), mean_b=kw.get("mean"), dw_b=kw.get("dw_b"), p_drop=kw.get("p_drop", 0.0),
                      seed=kw.get("seed", 0), dbias=kw.get("dbias"))
        if pn.mod is not None or kw.get("gate_idx") is not None:   # adaLN-Zero: modulated norm and / or gated branch, still one pass per row
            out = K.norm_residual_bwd_ada(pn.dy, pn.x, pn.rstd, pn.mean, pn.w, nt, S.L, dx, pn.dw, branch, **common, mod_n=pn.mod, dmod_n=pn.dmod, mod_idx=pn.mod_idx,
                                          modality=S.modality, any_img=S.any_img, mod_r=kw.get("mod"), dmod_r=kw.get("dmod"), gate_idx=kw.get("gate_idx"),
                                          modality_r=kw.get("modality"))
        else:
            out = K.norm_residual_bwd(pn.dy, pn.x, pn.rstd, pn.mean, pn.w, nt, S.L, dx, pn.dw, branch, **common)
        self._finish_block(bp, pn.finish, pn.dmod)
        return out

    def _block_backward(self, bp, i):
        S, G, lin, blk, nt, tc, sw = bp.S, bp.G, self._lins, self.blocks[i], bp.nt, self.time_conditioning, self.sandwich_normalization
        B, L, p_drop, seed0, R = S.B, S.L, S.p_drop, S.seed0, S.blocks[i]
        M, d, H, D, dev = B * L, self.hidden_size, self.n_heads, self.head_dim, S.ids.device
        if R.ckpt:   # activation checkpointing: rebuild this block's activations from its saved input, right before they are consumed
            with torch.no_grad():
                R = self._block_forward(S, i, R.x_in, None, last_rows=R.rows_c, recompute=True)[2]
        at, mod = blk.attention, R.mod
        dmod = torch.zeros((S.Bp, 6 * d), dtype=F32, device=dev) if tc else None
        f1, f2 = lin[f"{i}.fc1"], lin[f"{i}.fc2"]
        # MLP branch, fused with the pending norm above it: the final norm or norm1 of block i + 1 (with adaLN: where the fused pass is in use).  Without adaLN the
        # mlp.2 bias gradient = column sums of du2 comes out of the same pass
        kw = dict(mod=mod, dmod=dmod, gate_idx=5, modality=S.modality) if tc else dict(dbias=G[id(f2.bias)])
        kw.update(w_b=blk.post_ff_norm.weight.detach() if sw else None, rstd=R.rstd_m, mean=R.mean_m, norm_type=nt, dw_b=G[id(blk.post_ff_norm.weight)] if sw else None,
                  p_drop=p_drop, seed=seed0 + 4 * i + 2)
        pend, bp.pend = bp.pend, None
        du2 = self._norm_branch_bwd(bp, pend, R.u2, **kw)
        # dgrad through mlp.2 with the GELU' multiply and the mlp.0 bias gradient (column sums of du1) fused into the epilogue
        du1 = K.gemm_nt(du2, f2.w16t, N=4 * d, epilogue=K.EPI_DGELU, aux=R.u1, bias=G[id(f1.bias)])
        lo, lq = lin[f"{i}.out"], lin[f"{i}.qkv"]
        # few-tile regime (every weight of the block is at most half a round of tiles: UniDisc-S): the four weight gradients wait for the end of the block's
        # backward and share ONE split-K launch + ONE reduce (K.gemm_tn_multi) instead of three split-K launches + four reduce passes
        multi = pair_out = None
        if (self.multi_wgrads and du2.is_cuda and not tc and R.rows_c is None and M % 64 == 0 and lo.bias is None and lq.bias is None
                and all(K.gemm_tn_wants_splitk(l_.out, l_.inp) and l_.out % 256 == 0 and l_.inp % 256 == 0 for l_ in (f1, f2, lo, lq))):
            multi = [(du2, R.g, f2), (du1, R.h2, f1)]
        if multi is None:
            self._wgrad(du2, R.g, f2, G, bias_done=not tc)
        dh2 = f1.dgrad(du1, du1.shape[0], S.dgrad_form.get(f"{i}.fc1"))
        if multi is None:
            self._wgrad(du1, R.h2, f1, G, bias_done=True)
        del du1, du2
        # norm2 backward + attention branch
        p2 = _PendingNorm(dy=dh2, x=R.x_mid, rstd=R.rstd2, mean=R.mean2, w=blk.norm2.weight.detach(), dw=G[id(blk.norm2.weight)], accumulate=True,
                          mod=mod, dmod=dmod, mod_idx=(3, 4))
        if sw:
            da = self._norm_branch_bwd(bp, p2, R.a_out, w_b=blk.pre_residual_norm.weight.detach(), rstd=R.rstd_a, mean=R.mean_a, norm_type=nt,
                                       dw_b=G[id(blk.pre_residual_norm.weight)])
        elif tc:
            da = self._norm_branch_bwd(bp, p2, R.a_out, mod=mod, dmod=dmod, gate_idx=2, p_drop=p_drop, seed=seed0 + 4 * i + 1)
        else:
            da = self._norm_branch_bwd(bp, p2, R.a_out, p_drop=p_drop, seed=seed0 + 4 * i + 1)
        do = lo.dgrad(da, da.shape[0], S.dgrad_form.get(f"{i}.out"))
        # The out-proj weight gradient (2048 x 2048: 64 tiles) waits for the qkv one (6144 x 2048: 192 tiles of 256 rows) where the two fill the chip
        # exactly once TOGETHER (K.gemm_tn_pair): one launch instead of 256 tiles of 192 rows + a split-K launch + its reduce pass; few tiles over a long
        # contraction (UniDisc-S: 27 + 9) share ONE split-K launch
        if R.rows_c is not None:   # back to all rows: the rows left out have a zero gradient in both the attention output and the residual stream
            self._wgrad(da, R.o_c, lo, G)
            do = torch.zeros((M, d), dtype=do.dtype, device=dev).index_copy_(0, R.rows_c, do)
            bp.dx = torch.zeros((M, d), dtype=F32, device=dev).index_copy_(0, R.rows_c, bp.dx)
        elif multi is not None:
            multi.append((da, R.o, lo))
        elif (self.pair_wgrads and da.is_cuda and lo.bias is None and lq.bias is None and lo.inp == lq.inp
                and K.gemm_tn_pair_ok(lq.out, lo.out, lq.inp, M)
                and ((lq.out // 256 + lo.out // 256) * (lq.inp // 256) % 256 == 0 or (lq.out // 256 + lo.out // 256) * (lq.inp // 256) <= 128)):
            pair_out = (da, R.o)
        else:
            self._wgrad(da, R.o, lo, G)
        dqkr, dqkv = torch.empty((M, 2 * d), dtype=BF16, device=dev), torch.empty((M, 3 * d), dtype=BF16, device=dev)
        K.attention_bwd(R.qkr, R.qkv, R.o, do, R.lse, dqkr, dqkv, B, L, H, D, S.sid, S.doc_ranges, q_prescaled=True, **self._attn_mask_kw, **S.attn_drop_kw(i))
        qn = self.qk_norm
        K.qknorm_rope_bwd(dqkr, R.qkv, dqkv, S.cos, S.sin, L, D, gq=at.q_norm.weight.detach() if qn else None, gk=at.k_norm.weight.detach() if qn else None,
                          stats=R.qstats, dgq=G[id(at.q_norm.weight)] if qn else None, dbq=G[id(at.q_norm.bias)] if qn else None,
                          dgk=G[id(at.k_norm.weight)] if qn else None, dbk=G[id(at.k_norm.bias)] if qn else None, q_scale=self.attn_q_scale)
        dh1 = lq.dgrad(dqkv, dqkv.shape[0], S.dgrad_form.get(f"{i}.qkv"))
        if multi is not None:
            multi.append((dqkv, R.h1, lq))
            if not K.gemm_tn_multi([(dy_, x_, G[id(l_.weight)]) for dy_, x_, l_ in multi]):
                for dy_, x_, l_ in multi:    # (shapes outside the shared launch: the plain calls)
                    self._wgrad(dy_, x_, l_, G, bias_done=True)
        elif pair_out is not None:
            K.gemm_tn_pair(dqkv, R.h1, G[id(lq.weight)], pair_out[0], pair_out[1], G[id(lo.weight)])
        else:
            self._wgrad(dqkv, R.h1, lq, G)
        # norm1 pairs with the MLP branch of block i - 1 (with adaLN: where the fused pass covers the shape); this block is finished after that pass
        pn = _PendingNorm(dy=dh1, x=R.x_in, rstd=R.rstd1, mean=R.mean1, w=blk.norm1.weight.detach(), dw=G[id(blk.norm1.weight)], accumulate=True,
                          mod=mod, dmod=dmod, mod_idx=(0, 1), finish=i)
        if tc and not bp.tc_fused:
            self._norm_backward(bp, pn)
        else:
            bp.pend = pn

    def _sigma_map_backward(self, bp):
        """c = silu(W2 silu(W0 te + b0) + b2)"""
        S, G, lin = bp.S, bp.G, self._lins
        dc16 = torch.empty((S.Bp, self.cond_dim), dtype=BF16, device=bp.dc.device)
        if bp.ada_buf is not None and bp.ada_off:   # dc += the partial input-gradient tiles this pass's adaLN_modulation backwards left behind
            bp.dc += bp.ada_buf[:bp.ada_off].sum(0)
        K.cast_f32_bf16(bp.dc, dc16)
        dl2 = K.silu_bwd(S.l2, dc16)
        ds1 = K.gemm_nt(dl2, lin["sig2"].w16t, N=lin["sig2"].inp)
        self._wgrad(dl2, S.s1, lin["sig2"], G)
        dl1 = K.silu_bwd(S.l1, ds1)
        self._wgrad(dl1, S.te, lin["sig0"], G)

    def _ada_backward(self, bp, dmod, lin: _Lin):
        """adaLN_modulation backward: dmod fp32 [Bp, n*d] (atomically accumulated) -> dW, db, dc += dmod W."""
        G, c = bp.G, bp.S.c
        if bp.ada_buf is not None and lin.w16 is not None:
            # one launch (round 5): the input gradient as a GEMM is M = Bp rows, ONE output tile, K = 6 d - a single workgroup walking 12 288 k took ~140 us per block
            tiles = K.small_batch_linear_bwd_tiles(lin.out)
            parts = bp.ada_buf[bp.ada_off:bp.ada_off + tiles]
            bp.ada_off += tiles
            K.small_batch_linear_bwd(dmod, c, lin.w16, G[id(lin.weight)], G[id(lin.bias)] if lin.bias is not None else None, dx_parts=parts)
            return
        dmod16 = torch.empty(dmod.shape, dtype=BF16, device=dmod.device)
        K.cast_f32_bf16(dmod, dmod16)
        self._wgrad(dmod16, c, lin, G)
        K.gemm_nt(dmod16, lin.w16t, out=bp.dc, N=lin.inp, beta=1.0)


class _DitFn(torch.autograd.Function):
    """One autograd node for the whole backbone (+ fused SUBS cross-entropy in "logp" mode)."""

    @staticmethod
    def forward(ctx, module: DIT, mode: str, inputs: _EngineInputs, *params):
        out, S = module._engine_forward(inputs, mode, save=bool(inputs.save))   # (grad mode is off inside Function.forward, so the caller decided)
        ctx.module, ctx.mode, ctx.S = module, mode, S if inputs.save else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.S is None:
            raise RuntimeError("unidisc_amd.DIT: backward called but activations were not saved")
        grads = ctx.module._engine_backward(ctx.S, grad_out, ctx.mode)
        ctx.S = None
        req = [p.requires_grad for p in ctx.module._ordered_params()]
        return (None, None, None, *[g if r else None for g, r in zip(grads, req)])
