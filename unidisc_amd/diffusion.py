"""Trainer-level hot path: the reference's ``model.py::Diffusion`` methods that run every training step.

Mirrors, with the same names / argument meaning / error behaviour:
  ``update_batch`` (model.py:157-395, token-dataset branch), ``get_cond_dict`` (:397-418), ``training_step`` (:420-422),
  ``q_xt`` (:424-587), ``_sample_t`` (:589-619), ``_subs_parameterization`` (:621-658), ``_process_sigma`` (:660-672),
  ``forward`` (:674-795), ``compute_loss`` (:797-1173) and the ``Loss`` record (model_utils.py:110-120).

Host logic (RNG draws, masks, weights, reductions on [B] / [B,L] tensors) is plain torch on the device — the
reference's draw order ``rand(B)`` → ``rand(B,L)`` → ``rand(B,1)``×2 is preserved so masks are bit-exact for a
given generator state.  All O(B·L·d) and O(B·L·V) work goes through ``unidisc_amd.DIT`` (HIP kernels).
``compute_loss`` uses the fused path ``backbone.forward_logp`` and never materialises [B,L,V] log-probs;
``forward`` still returns full SUBS log-probs (or logits) for samplers.
"""
from __future__ import annotations

import math
import os

from collections import namedtuple
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import kernels as K
from .dit import DIT, ModalityMask, cfg_get, static_modality
from .noise_schedule import LogLinearNoise, get_noise


@dataclass
class Loss:  # model_utils.py:110-120
    loss: torch.FloatTensor
    img_loss: torch.FloatTensor = None
    txt_loss: torch.FloatTensor = None
    nlls: torch.FloatTensor = None
    token_mask: torch.FloatTensor = None
    txt_nlls: torch.FloatTensor = None
    img_nlls: torch.FloatTensor = None
    extra_losses: dict = None
    modality_mask: torch.FloatTensor = None


class _LinearLoss(torch.autograd.Function):
    """loss(log_p) with a precomputed value and gradient coefficient: the diffusion loss is linear in the per-token log-probabilities"""

    @staticmethod
    def forward(ctx, log_p, coef, value):
        ctx.save_for_backward(coef)
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        (coef,) = ctx.saved_tensors
        return (g * coef).to(coef.dtype), None, None


# ---- the records of the host sampler (Diffusion.sample and the methods around it, below)
class MaskedLogits(NamedTuple):
    """The logits of the [MASK] rows of one forward, every tensor already cut to its n rows: logits [n, Vp], rows [n] (flat indices into [B, L]), and with
    guidance the unconditional half's logits_u [n, Vp] on the same rows and the guidance weight of every row, w_rows [n] (both None without guidance).
    The samplers keep it as their cache while x does not change (the reference's p_x0 cache)."""
    logits: torch.Tensor
    rows: torch.Tensor
    n: int
    logits_u: Optional[torch.Tensor] = None
    w_rows: Optional[torch.Tensor] = None

    @classmethod
    def of(cls, logits, rows, n):
        """from what `DIT.forward_masked_logits` returns: the [MASK] rows first, then padding rows"""
        return cls(logits[:n], rows[:n], n)


# `Diffusion.sample`'s predictors: the update method, the mode of its unmasking schedule (None: it has none and keeps a logits cache instead), the keywords
# its pair of recorded draws is passed as, whether it takes the fused step tail (`tail=`) and whether the tensor tail has anything to write back after it
_Predictor = namedtuple("_Predictor", "update schedule draws fuses_tail writes_back")
_PREDICTORS = {
    "ddpm_cache": _Predictor("_ddpm_cache_step", None, None, False, True),
    "maskgit": _Predictor("_maskgit_update", "arccos", ("pred", "gumbel"), True, True),
    "maskgit_nucleus": _Predictor("_maskgit_nucleus_update", "arccos", ("pred", "gumbel"), True, True),
    "first_hitting": _Predictor("_first_hitting_update", "linear", ("u", "pos_u"), True, False),   # (the update leaves every given position alone)
}


class _SamplerState:
    """What the sampler loop mutates - x, the conditioning x0 / x0_unmask, the modality map, the EOS rule's modality map and the logits cache - with the one way
    to run on a slice of the positions: `narrow(sl)` keeps the full tensors and continues on their columns sl, `widen()` writes the slice's x back into the
    full x and restores the rest.  eval.attention_caching narrows to the text and widens again every few steps, eval.conditioning_cache narrows once."""

    def __init__(self, x, x0, x0_unmask, modality, eos_mod):
        self.x, self.x0, self.x0_unmask, self.modality, self.eos_mod = x, x0, x0_unmask, modality, eos_mod
        self.cache, self._full = None, None

    @property
    def narrowed(self):
        return self._full is not None

    def narrow(self, sl, modality):
        """`modality`: the map the slice's rows read (the state's own, or the static slices written out)"""
        cut = (lambda v: None if v is None else v[:, sl].contiguous())
        self._full = (sl, self.x.clone(), self.x0, self.x0_unmask, self.modality, self.eos_mod, self.cache)
        self.cache = Diffusion._cache_to_slice(self.cache, self.x.shape[1], sl)
        self.x, self.x0, self.x0_unmask, self.modality, self.eos_mod = cut(self.x), cut(self.x0), cut(self.x0_unmask), cut(modality), cut(self.eos_mod)

    def widen(self, keep_cache=False):
        """keep_cache: the full cache saved by narrow() takes the slice's current cache back (`_cache_to_full`: a text slice); otherwise the cache is dropped"""
        sl, x_full, self.x0, self.x0_unmask, self.modality, self.eos_mod, cache_full = self._full
        x_full[:, sl] = self.x
        self.cache = Diffusion._cache_to_full(cache_full, self.cache, x_full.shape[1], sl.stop) if keep_cache else None
        self.x, self._full = x_full, None


def _seed_or_default(seed):
    return int(seed if seed is not None else torch.initial_seed())


class Diffusion:
    def __init__(self, config, tokenizer, device, disable_init=False, backbone: Optional[torch.nn.Module] = None):
        self.config, self.tokenizer, self.device = config, tokenizer, torch.device(device)
        if disable_init:
            return
        self.init(config, tokenizer, device, backbone)

    # ---- model_setup.init (model_setup.py:47-327), hot-path subset
    def init(self, config, tokenizer, device, backbone=None):
        m, tr = cfg_get(config, "model"), cfg_get(config, "trainer")
        self.global_step = 0
        self.current_run_fwd_bwd_pass = 0
        prec = str(cfg_get(tr, "precision", "bf16"))
        self.dtype = torch.float32 if ("fp32" in prec or "no" in prec) else (torch.bfloat16 if "bf16" in prec else torch.float16)
        if self.dtype != torch.bfloat16:
            raise NotImplementedError(f"unidisc_amd: trainer.precision={prec}; only bf16 (the reference's training precision) is implemented in HIP")
        # trainer options that change the loss / the batch and are not built: refuse them instead of training silently with another objective
        for flag, why in (("ar_llm_loss", "the extra auto-regressive LLM loss term (model.py:1076-1136)"),
                          ("force_remove_img_tokens", "dropping image tokens from the batch (model.py:316-319, :1054)"),
                          ("add_label", "the class-label token written by update_batch (model.py:321-334)")):
            if cfg_get(tr, flag, False):
                raise NotImplementedError(f"unidisc_amd: trainer.{flag} — {why} — is not on the denoising hot path (SURVEY.md §8)")
        # trainer.low_precision_loss (model.py:747, :924) keeps the SUBS log-probabilities in the autocast dtype instead of widening them to fp32 before the gather.  Under
        # bf16 autocast they ARE bf16 values either way (widening is exact) and every later product meets an fp32 weight, so the reference's loss is the same number with
        # the flag on or off; this path takes log p from an fp32 log-sum-exp in both cases.  Accepted, nothing to switch.
        self.image_model = bool(cfg_get(m, "image_model", False))
        self.unified_model = bool(cfg_get(m, "unified_model", False))
        self.antithetic_sampling = cfg_get(tr, "antithetic_sampling", True)
        self.importance_sampling = cfg_get(tr, "importance_sampling", False)
        self.change_of_variables = cfg_get(tr, "change_of_variables", False)
        if self.importance_sampling or self.change_of_variables:
            raise NotImplementedError("unidisc_amd: importance_sampling / change_of_variables are off in every shipped config and not implemented")
        if self.image_model is False or self.unified_model:  # model_setup.py:89-98
            forced = cfg_get(m, "force_text_vocab_size", None)
            self.vocab_size = forced if forced is not None else len(tokenizer)
            if tokenizer is None or getattr(tokenizer, "mask_token", None) is None:
                self.mask_index = self.vocab_size
                self.vocab_size += 1
            else:
                self.mask_index = tokenizer.mask_token_id
        if self.image_model:  # :99-113
            if self.unified_model:
                self.text_vocab_size = self.vocab_size
                self.vocab_size += cfg_get(m, "image_vocab_size")
                self.image_vocab_size = cfg_get(m, "image_vocab_size")
            else:
                self.vocab_size = cfg_get(m, "image_vocab_size") + 1
                self.mask_index = self.vocab_size - 1
                self.text_vocab_size = 0
        else:
            self.text_vocab_size = self.vocab_size
        self.parameterization = cfg_get(config, "parameterization", "subs")
        if self.parameterization not in ("subs", "ar"):
            raise NotImplementedError(f"unidisc_amd: parameterization={self.parameterization}; SUBS and the AR baseline (ar) are implemented")
        if self.parameterization == "ar":
            self._check_ar(config, m, tr)
        if cfg_get(config, "backbone", "dit") != "dit":
            raise NotImplementedError("unidisc_amd: only backbone=dit is implemented")
        self.static_txt_sl = slice(None, cfg_get(m, "txt_length"))
        self.static_img_sl = slice(-cfg_get(m, "img_length"), None) if cfg_get(m, "img_length", 0) else slice(0, 0)
        if backbone is None:  # model_setup.py:148-161
            backbone = DIT(config, vocab_size=self.vocab_size, text_vocab_size=self.text_vocab_size, mask_index=self.mask_index, autocast_dtype=self.dtype,
                           device=device, static_img_sl=self.static_img_sl, static_txt_sl=self.static_txt_sl)
        self.backbone = backbone
        self.T = cfg_get(config, "T", 0)
        if self.T:
            raise NotImplementedError("unidisc_amd: discrete-time T>0 (D3PM loss) is not on the denoising hot path")
        self.noise = get_noise(config)
        self.sampling_eps = cfg_get(tr, "sampling_eps", 1e-3)
        self.time_conditioning = cfg_get(config, "time_conditioning", False)
        self.neg_infinity = -1000000.0  # model_setup.py:269

    @staticmethod
    def _check_ar(config, m, tr):
        """The AR baseline as configs/experiments/ar.yaml trains it (parameterization=ar, trainer.ar_shift, model.full_attention=false): next-token
        cross-entropy, no time conditioning, x_t = x_0.  The AR variants of the trainer that change the batch or the objective are not built."""
        if cfg_get(config, "time_conditioning", False) or cfg_get(m, "force_time_conditioning", False):
            raise NotImplementedError("unidisc_amd: parameterization=ar with time_conditioning - the AR baseline has no sigma (model.py:840-918)")
        if not cfg_get(tr, "ar_shift", False):
            raise NotImplementedError("unidisc_amd: parameterization=ar without trainer.ar_shift (unshifted AR training) is not built")
        for flag, why in (("rand_ar_modality_dropout", "masking a sample's first modality (model.py:906-913)"),
                          ("ar_inpainting", "the doubled inpainting sequence (model.py:884-900)"),
                          ("rand_flip_ar_prob", "flipping the modality order of a batch (model.py:357-380)"),
                          ("ar_llm_loss", "the extra LLM loss term (model.py:1076-1136)"),
                          ("use_orig_unidisc_dit", "the original UniDisc DiT head (model.py:757)")):
            if cfg_get(tr, flag, None) not in (None, False):
                raise NotImplementedError(f"unidisc_amd: parameterization=ar with trainer.{flag} - {why} - is not built")

    rng_device = None  # set to "cpu" to draw t / masks from the CPU generator (bit-reproducible across devices)
    _generic_qxt = False   # tests: route q_xt through the tensor statements even where the fused launch applies

    def _rand(self, *shape, device):
        if self.rng_device is None:
            return torch.rand(*shape, device=device)
        return torch.rand(*shape, device=self.rng_device).to(device)

    @property
    def training(self):
        return self.backbone.training

    @property
    def allow_slicing(self):  # model.py:1283-1285
        return not self.backbone.training

    def txt_sl(self, batch=None):
        return batch["modality_mask"][..., 0]

    def img_sl(self, batch=None):
        return batch["modality_mask"][..., 1]

    # ---- the batch contract of model.py:157-395 (token-dataset and pre-tokenised branches), in this module's own structure
    def update_batch(self, batch):
        """Dataset batch -> model batch.  Output keys and values are the reference's (`input_ids`, `attention_mask`, `modality`, `modality_mask`,
        `batch_contains_img`, `txt_sl`, `img_sl`, `sample_ids`), produced in three stages:
          1. everything onto the device in the DATASET's dtypes (80 KiB per step at 1.4 B), so that
          2. the joint sequence comes from ONE gather launch (`_assemble_on_device`, tokens.hip) wherever the batch has the token-dataset shape, and from
             `_joint_sequence_generic` (slice writes into preallocated tensors) for the shapes the kernel does not cover;
          3. modality / attention-mask / sample-id fields derived without in-place edits of the caller's tensors."""
        if batch is None:
            return batch
        cfg, tr, m = self.config, cfg_get(self.config, "trainer"), cfg_get(self.config, "model")
        data = cfg_get(cfg, "data")
        out = {}
        for key, val in (batch.items() if not isinstance(batch, dict) else dict(batch).items()):
            if isinstance(val, (list, tuple)) and val and all(isinstance(v, torch.Tensor) for v in val) and key in ("img_input_ids", "txt_input_ids", "sample_ids"):
                val = torch.stack(list(val), dim=0)
            out[key] = val.to(self.device) if isinstance(val, torch.Tensor) else val
        fused = False
        if self.image_model or cfg_get(data, "force_image_dataset", False):
            has_token_fields = "txt_input_ids" in out or "img_input_ids" in out
            assembled = "input_ids" in out and "modality" in out
            if "img" in out and not has_token_fields:
                raise NotImplementedError("unidisc_amd: raw-image batches need the VQ tokenizer, which is outside the denoising hot path")
            if has_token_fields:
                fused = self._assemble_on_device(out, tr, m)
                if not fused:
                    self._joint_sequence_generic(out, tr, m)
            elif cfg_get(tr, "multimodal_batches", False) or assembled:
                # pre-tokenised multimodal batches, and batches token_data.TokenBatcher assembled on the device already
                out["input_ids"] = out["input_ids"].long()
                if cfg_get(tr, "force_shift_image_batches", False):
                    out["input_ids"] = out["input_ids"] + (out["modality"] == 1).long() * self.text_vocab_size
            else:
                raise NotImplementedError("unidisc_amd: raw-image batches need the VQ tokenizer, which is outside the denoising hot path")
            if out["input_ids"].shape[1] != cfg_get(m, "length") and not cfg_get(tr, "ar_inpainting", False):
                raise AssertionError(f"input ids are not the correct length input ids shape: {out['input_ids'].shape}, model length: {cfg_get(m, 'length')}")
        if "sample_ids" in out:
            out["sample_ids"] = out["sample_ids"].long()
        self._modality_fields(out, tr, m, data, checked=fused)
        self._attention_fields(out, tr, data)
        return out

    def _joint_sequence_generic(self, b, tr, m):
        """`input_ids` / `attention_mask` / `modality` of a token batch the gather kernel does not take (host-dtype surprises, text-less or user-supplied
        modality, CPU tests): [text | image + Vt] written into preallocated [B, Lt + Li] tensors."""
        img = b.pop("img_input_ids")
        txt = b.get("txt_input_ids")
        B, Li = img.shape[0], img.shape[-1]
        Lt = txt.shape[-1] if txt is not None else 0
        ids = torch.empty((B, Lt + Li), dtype=torch.int64, device=img.device)
        keep = torch.ones((B, Lt + Li), dtype=torch.bool, device=img.device)
        ids[:, Lt:] = img
        if txt is not None:   # image ids live behind the text vocabulary only in a joint sequence
            b["txt_input_ids"] = txt.long()
            ids[:, Lt:] += self.text_vocab_size
            ids[:, :Lt] = txt
            keep[:, :Lt] = b["txt_attention_mask"]
        b["input_ids"], b["attention_mask"] = ids, keep
        if "modality" not in b:
            if cfg_get(tr, "ignore_text_in_unified", False):
                b["modality"] = torch.ones_like(ids)
            else:
                if not (cfg_get(m, "txt_length") > 0 and cfg_get(m, "img_length") > 0):
                    raise AssertionError("a token batch without `modality` needs model.txt_length > 0 and model.img_length > 0")
                b["modality"] = (torch.arange(Lt + Li, device=ids.device) >= Lt).long().expand(B, -1).contiguous()

    def _modality_fields(self, b, tr, m, data, checked=False):
        mm = cfg_get(tr, "multimodal_batches", False)
        mod = b.get("modality")
        if mod is not None:
            mod = mod.long()
            if mm and mod.ndim == 2 and mod.shape[-1] == 1:    # one modality per sample -> per token
                mod = mod.expand(-1, cfg_get(m, "length")).contiguous()
        elif self.image_model and not mm:                     # static layout: the image occupies the last img_length positions
            mod = self._static_modality(*b["input_ids"].shape, b["input_ids"].device)
        elif cfg_get(data, "txt_only", False):
            mod = torch.zeros_like(b["input_ids"], dtype=torch.int64)
        if mod is None:
            return
        if not checked:   # (the gather kernel writes 0 / 1 by construction)
            mod = mod.clamp_min(0)          # padding (-1, PackingCollate) counts as text
            self._check_modality_range(mod)
        b["modality"] = mod
        is_img = mod == 1
        b["modality_mask"] = torch.stack((~is_img, is_img), dim=-1)     # == one_hot(modality, 2).bool() once the range check holds
        b["batch_contains_img"] = is_img.any(dim=-1)
        b["txt_sl"], b["img_sl"] = self.txt_sl(b), self.img_sl(b)

    def _attention_fields(self, b, tr, data):
        am = b["attention_mask"]
        am = torch.ones_like(am, dtype=torch.bool) if cfg_get(tr, "force_full_attention_mask", False) else am.to(torch.bool)
        if cfg_get(data, "require_sample_ids", False):
            if "sample_ids" not in b:
                raise AssertionError("data.require_sample_ids: the batch has no `sample_ids`")
            sid = torch.where(am, b["sample_ids"], torch.full_like(b["sample_ids"], -1))     # padding belongs to no sample ...
            am = am & (sid != -1)                                                             # ... and a position without a sample is padding
            b["sample_ids"] = sid
        b["attention_mask"] = am
        if cfg_get(tr, "interleaved", False) and "sample_ids" not in b:
            b["sample_ids"] = torch.zeros_like(b["modality"], dtype=torch.int64)

    def _assemble_on_device(self, batch, tr, m):
        """model.py:183-212 for a token batch that is already on the device in the dataset's own dtypes (int32 text, int16 image ids, bool text mask): joint ids
        (image ids shifted by the text vocabulary), attention mask (text mask | ones) and modality map in ONE launch (tokens.hip, the TokenBatcher's kernel) instead
        of nine tensor statements.  Same values bit for bit; `txt_input_ids` stays in the batch as int64 like in the reference."""
        txt, img, tm = batch.get("txt_input_ids"), batch.get("img_input_ids"), batch.get("txt_attention_mask")
        ok = (isinstance(txt, torch.Tensor) and isinstance(img, torch.Tensor) and isinstance(tm, torch.Tensor) and txt.is_cuda and img.is_cuda and tm.is_cuda
              and txt.dtype == torch.int32 and img.dtype == torch.int16 and tm.dtype == torch.bool and txt.dim() == 2 and img.dim() == 2 and tm.shape == txt.shape
              and txt.is_contiguous() and img.is_contiguous() and tm.is_contiguous() and txt.shape[0] == img.shape[0]
              and "modality" not in batch and "sample_ids" not in batch and "attention_mask" not in batch and "input_ids" not in batch
              and not cfg_get(tr, "ignore_text_in_unified", False) and cfg_get(m, "txt_length") > 0 and cfg_get(m, "img_length") > 0)
        if not ok:
            return False
        ids, mask, modality = K.assemble_joint_tokens(txt, tm, img, self.text_vocab_size)
        batch.pop("img_input_ids")
        batch["txt_input_ids"] = txt.to(torch.int64)
        batch["input_ids"], batch["attention_mask"], batch["modality"] = ids, mask, modality
        return True

    _checks = ()   # queued device-side batch checks: (event, pinned result)

    def _check_modality_range(self, modality):
        """model.py:311 `assert modality.min() == 0 and modality.max() == 1`.  On the device the reference's form is a host synchronisation at the top of
        EVERY step (the host can never run ahead of the GPU across a step boundary: measured 0.5 ms of idle GPU per 88 ms step at 1.4 B, 2.7 ms per 31 ms
        step at UniDisc-S).  Here the two extrema are queued to pinned memory and the same AssertionError is raised at the step's first natural host wait
        (`_flush_checks`, called after the backbone forward and at the next `update_batch`), before any gradient of that batch is used."""
        self._flush_checks()
        if not modality.is_cuda or os.environ.get("UDM_SYNC_CHECKS") == "1":   # (the knob: the reference's immediate, synchronising form)
            assert modality.min() == 0 and modality.max() == 1
            return
        lo, hi = torch.aminmax(modality)
        host = torch.empty(2, dtype=modality.dtype).pin_memory()
        host.copy_(torch.stack((lo, hi)), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._checks = list(self._checks) + [(ev, host)]

    def _flush_checks(self):
        checks = self._checks
        if not checks:
            return
        self._checks = ()
        for ev, host in checks:
            ev.synchronize()
            assert int(host[0]) == 0 and int(host[1]) == 1, f"batch['modality'] must contain both 0 and 1 and nothing else (min {int(host[0])}, max {int(host[1])})"

    def get_cond_dict(self, batch):  # model.py:397-418
        ret = dict()
        if "cond_input_ids" in batch or "img_label" in batch:
            raise NotImplementedError("unidisc_amd: image / label conditioning is outside the denoising hot path")
        if cfg_get(cfg_get(self.config, "model"), "use_attention_mask", False):   # model.py:405-406: the padding mask goes to the backbone's attention (a key mask)
            ret["attention_mask"] = batch["attention_mask"]
        if cfg_get(cfg_get(self.config, "trainer"), "multimodal_batches", False):
            ret["modality"] = batch["modality"]
        return ret

    def training_step(self, batch, batch_idx):  # model.py:420-422
        batch = self.update_batch(batch)
        return self.compute_loss(batch, prefix="train", batch_idx=batch_idx)

    # ---- forward corruption q(x_t | x_0), absorbing state (contract of model.py:424-587)
    def q_xt(self, x, move_chance, allow_move_mask=None, return_ignore_batch_mask_for_metrics=False, mask_image_square=False, mask_text_region=False,
             batch=None):
        """x_t = [MASK] where a position "moves", x_0 elsewhere.  A position moves when its uniform falls below the sample's move chance; in training a
        sample's whole text (or image) side may be masked instead (`trainer.mask_entire_modality`).  Draw order - rand(B, L), then the per-sample draws, then
        (interleaved) one draw per block - is the reference's, so masks are bit-exact for a given generator state.
        Returns x_t, or (x_t, ignore_batch_mask_for_metrics, None, should_mask_txt, should_mask_img, move_indices)."""
        tr = cfg_get(self.config, "trainer")
        if mask_image_square or mask_text_region:
            raise NotImplementedError("unidisc_amd: square / region masking are evaluation-time options outside the hot path")
        for flag in ("joint_ar_nar_prob", "first_token_dropout"):
            if cfg_get(tr, flag, None) is not None:
                raise NotImplementedError(f"unidisc_amd: trainer.{flag} is not on the denoising hot path")
        if cfg_get(tr, "discrete_diffusion_mode", "absorbing") != "absorbing":
            raise NotImplementedError("unidisc_amd: only absorbing-state diffusion is implemented")
        r_move = self._rand(*x.shape, device=x.device)
        mask_prob = cfg_get(tr, "mask_entire_modality", None)
        whole = mask_prob is not None and self.backbone.training
        multimodal, interleaved = cfg_get(tr, "multimodal_batches", False), cfg_get(tr, "interleaved", False)
        if whole and batch is None:
            raise AssertionError("q_xt: trainer.mask_entire_modality needs the batch (modality masks)")
        # per-sample uniforms of the whole-modality lottery: text first, image second (none for the image side under mask_txt_only)
        r_txt = r_img = None
        p_txt = p_img = 0.0
        if whole:
            r_txt = self._rand(x.shape[0], 1, device=x.device)
            if cfg_get(tr, "mask_txt_only", False):
                p_txt = mask_prob
            else:
                r_img = self._rand(x.shape[0], 1, device=x.device)
                p_txt = p_img = mask_prob / 2

        kernel_ok = (not self._generic_qxt and x.dim() == 2 and x.dtype == torch.int64 and move_chance.numel() == x.shape[0] and not (whole and (interleaved or not multimodal)))
        if kernel_ok:
            # comparisons and selects on [B, L] / [B, 1] as ONE launch (udm_qxt_absorbing): per-token move, the lottery with its both-sides-drawn rule,
            # the row REPLACEMENT by the modality mask, x_t
            xt, move, smt, smi, ignore = K.qxt_absorbing(x.contiguous(), r_move.float().contiguous(), move_chance.float(), self.mask_index, r_txt=r_txt, r_img=r_img,
                                                         p_txt=p_txt, p_img=p_img, modality_mask=batch["modality_mask"].contiguous() if whole else None)
            if allow_move_mask is not None:    # positions the caller protects never move (applied after the lottery)
                move = move & allow_move_mask
                xt = torch.where(move, self.mask_index, x)
            return (xt, ignore, None, smt, smi, move) if return_ignore_batch_mask_for_metrics else xt

        move = r_move < move_chance
        smt = smi = ignore = None
        if whole:
            smt = r_txt < p_txt
            smi = (r_img < p_img) if r_img is not None else torch.zeros_like(smt)
            if interleaved and multimodal:
                block_move, ignore = self._interleaved_block_lottery(batch, mask_prob, x.shape, x.device)
                move = move | block_move
                if allow_move_mask is not None:    # protected positions never move, whole-block masks included (model.py:564-565 sits behind every branch)
                    move = move & allow_move_mask
                xt = torch.where(move, self.mask_index, x)
                return (xt, ignore, None, smt, smi, move) if return_ignore_batch_mask_for_metrics else xt
            # a sample that drew BOTH sides keeps its per-token mask
            both = smt & smi
            smt, smi = smt & ~both, smi & ~both
            if multimodal:    # the row's mask is REPLACED: "all text masked, all image clean" (or the reverse)
                txt_cols, img_cols = batch["modality_mask"][..., 0], batch["modality_mask"][..., 1]
                move = torch.where(smt, txt_cols, torch.where(smi, img_cols, move))
            else:             # static layout: the side is masked ON TOP of the per-token mask; a text-only sample has no image side to mask
                smi = smi & ~batch["txt_sl"].all(dim=-1, keepdim=True)
                cols = torch.arange(x.shape[1], device=x.device)
                txt_cols = torch.zeros(x.shape[1], dtype=torch.bool, device=x.device)
                img_cols = torch.zeros_like(txt_cols)
                txt_cols[cols[self.static_txt_sl]] = True
                img_cols[cols[self.static_img_sl]] = True
                move = move | (smt & txt_cols) | (smi & img_cols)
            ignore = smt | smi
        if allow_move_mask is not None:
            move = move & allow_move_mask
        xt = torch.where(move, self.mask_index, x)
        return (xt, ignore, None, smt, smi, move) if return_ignore_batch_mask_for_metrics else xt

    def _interleaved_block_lottery(self, batch, mask_prob, shape, dev):
        """Packed / interleaved rows (model.py:483-522): every (modality, packed sample) block of more than 4 tokens is masked as a whole with probability
        2 p (k + 1) / n  (k: index of the block inside its sample, n: blocks of that sample); one uniform per block, drawn after the two per-row draws
        (the reference's call order).  Everything stays on the device; the ONE host read is the number of candidate blocks (it sizes the uniform draw - the
        reference reads every block boundary back).  Blocks are numbered in (row, position) order, the order of the reference's draws.
        Returns (block mask [B, L], rows that had a block masked [B])."""
        batch_size, seq_len = shape
        mod, sid = batch["modality"], batch["sample_ids"]
        x_is_cuda = mod.is_cuda
        if x_is_cuda and os.environ.get("UDM_INTERLEAVED_KERNELS", "1") != "0":
            # two launches (udm_interleaved_block_lottery, tokens.hip) instead of ~40 tensor statements with a sort and three contended scatter_adds; bit-identical to the
            # statements below (tests/test_gpu_kernels.py).  Device generator: one uniform per POSSIBLE candidate (a candidate block is longer than 4 tokens: at most
            # seq_len // 5 per row), no host read.  Replay (rng_device = "cpu"): the reference draws exactly n_cand uniforms, so the count is read back first.
            if self.rng_device is None:
                r = self._rand(batch_size * (seq_len // 5 + 1), 1, device=dev)
            else:
                _, _, n_dev = K.interleaved_block_lottery(mod, sid, torch.empty(0, device=dev), mask_prob)
                n_cand = int(n_dev)
                if not n_cand:
                    return torch.zeros((batch_size, seq_len), dtype=torch.bool, device=dev), torch.zeros((batch_size,), device=dev, dtype=torch.bool)
                r = self._rand(n_cand, 1, device=dev)
            accum, rows_hit, _ = K.interleaved_block_lottery(mod, sid, r, mask_prob)
            return accum, rows_hit
        N = batch_size * seq_len
        chg = torch.ones((batch_size, seq_len), dtype=torch.bool, device=dev)
        chg[:, 1:] = (mod[:, 1:] != mod[:, :-1]) | (sid[:, 1:] != sid[:, :-1])
        gid = chg.reshape(-1).cumsum(0) - 1                                          # block of every position
        one = torch.ones(N, dtype=torch.int64, device=dev)
        ar = torch.arange(N, device=dev)
        blen = torch.zeros(N, dtype=torch.int64, device=dev).scatter_add_(0, gid, one)
        bsid = torch.full((N,), -1, dtype=torch.int64, device=dev).scatter_(0, gid, sid.reshape(-1))
        brow = torch.zeros(N, dtype=torch.int64, device=dev).scatter_(0, gid, ar // seq_len)
        cand = (bsid >= 0) & (blen > 4)
        if self.rng_device is None and x_is_cuda:
            # device generator (production): one uniform per POSSIBLE candidate block - at most seq_len // 5 per row, blocks being longer than 4 - indexed by the
            # candidate's rank, so the host never reads the count back (that read stalled the launch queue at the top of every step: 2.7 ms of idle GPU per 81 ms
            # step of the packed 4608-token workload).  The draws of a block do not depend on how many follow it; the stream position after the step differs from a
            # draw of exactly n_cand values, which only a bit-exact REPLAY needs - and replays run with rng_device = "cpu" (below: the exact count).
            n_cand = batch_size * (seq_len // 5 + 1)
        else:
            n_cand = int(cand.sum())
            if not n_cand:
                return torch.zeros((batch_size, seq_len), dtype=torch.bool, device=dev), torch.zeros((batch_size,), device=dev, dtype=torch.bool)
        # k = index of the block among the candidate blocks of its (row, sample id), n = their number: stable sort by that key
        key = torch.where(cand, brow * (seq_len + 1) + bsid, torch.full_like(brow, (batch_size + 1) * (seq_len + 1)))
        order = torch.argsort(key, stable=True)
        skey = key[order]
        newg = torch.ones(N, dtype=torch.bool, device=dev)
        newg[1:] = skey[1:] != skey[:-1]
        g_first = torch.cummax(torch.where(newg, ar, torch.zeros_like(ar)), 0).values
        g_id = newg.cumsum(0) - 1
        g_size = torch.zeros(N, dtype=torch.int64, device=dev).scatter_add_(0, g_id, one)
        k = torch.empty_like(ar).scatter_(0, order, ar - g_first)
        n = torch.empty_like(ar).scatter_(0, order, g_size[g_id])
        r = self._rand(n_cand, 1, device=dev).reshape(-1)
        r_blk = r[(cand.cumsum(0) - 1).clamp(min=0)]
        thr = mask_prob * ((k + 1) / n) * 2                                      # fp32, in the reference's order of operations
        hit = cand & (r_blk < thr)
        rows_hit = torch.zeros(batch_size, dtype=torch.int64, device=dev).scatter_add_(0, brow, hit.long()) > 0
        return hit[gid].reshape(batch_size, seq_len), rows_hit

    def _sample_t(self, n, device):
        """Diffusion times of a batch (contract of model.py:589-619): t = eps_s + (1 - eps_s) u with u ~ U[0, 1), stratified over the batch when
        `antithetic_sampling` (sample i owns the i-th of n equal strata).  The GPU step gets the same values from `udm_sample_t_noise`."""
        tr = cfg_get(self.config, "trainer")
        if cfg_get(tr, "joint_ar_nar_timestep_warmup_steps", None) is not None:
            raise NotImplementedError("unidisc_amd: joint AR/NAR timestep warm-up is not on the denoising hot path")
        u = self._rand(n, device=device)
        if self.antithetic_sampling:
            u = torch.remainder(u / n + torch.arange(n, device=device) / n, 1)
        forced = cfg_get(tr, "force_timestep", None)
        if forced is not None:
            u = torch.full_like(u, forced)
        return (self.sampling_eps + (1 - self.sampling_eps) * u).to(torch.float32)

    def _restrict(self):
        return bool(cfg_get(cfg_get(self.config, "model"), "force_argmax_valid_indices", False))

    def _subs_parameterization(self, logits, xt, batch=None, modality=None, **kwargs):
        """model.py:621-658 on the HIP path: bf16 logits [B,L,V] -> SUBS log-probs [B,L,V] (same dtype)."""
        B, L, V = logits.shape
        flat = logits.reshape(B * L, V)
        if flat.stride(0) % 8 != 0 or flat.stride(1) != 1 or flat.data_ptr() % 16 != 0 or flat.dtype != torch.bfloat16:
            buf = torch.zeros((B * L, (V + 7) // 8 * 8), dtype=torch.bfloat16, device=logits.device)
            buf[:, :V] = flat
            flat = buf
        mod = modality
        if self._restrict() and mod is None and batch is not None and cfg_get(cfg_get(self.config, "trainer"), "multimodal_batches", False):
            mod = batch["modality"]
        if self._restrict() and mod is None:  # static slices (model.py:634-635)
            mod = self._static_modality(B, L, logits.device)
        out = K.subs_logprobs(flat, xt.reshape(-1).contiguous() if xt is not None else None, mod.reshape(-1).contiguous() if mod is not None else None, V,
                              self.text_vocab_size, self.mask_index, self._restrict(), out_dtype=logits.dtype if logits.dtype == torch.float32 else torch.bfloat16)
        return out.view(B, L, V)

    def _process_sigma(self, sigma):  # model.py:660-672
        if sigma is None:
            assert cfg_get(cfg_get(self.config, "trainer"), "allow_null_sigma", False)
            return sigma
        if sigma.ndim > 1:
            sigma = sigma.squeeze(-1)
            assert sigma.ndim == 1, sigma.shape
        if not self.time_conditioning and cfg_get(cfg_get(self.config, "model"), "force_time_conditioning", False):
            sigma = torch.zeros_like(sigma)
        return sigma

    def forward(self, x, sigma, batch=None, forward_attention_mask=None, return_additional_loss=False, x_img_emb=None, disable_ar_shift=False,
                continuous_mode=False, joint_ar_nar_mask=None, return_logits=False, block_mask=None, update_cache_slice=None, **kwargs):
        """Returns log score (model.py:674-795): SUBS log-probs [B,L,V] (bf16), or raw logits when ``return_logits``.  AR baseline: next-token log-probs
        [B, L-1, V] (trainer.ar_shift), or [B, L, V] with ``disable_ar_shift``."""
        sigma = self._process_sigma(sigma)
        if self.parameterization == "ar":
            return self._ar_forward(x, batch, return_logits, disable_ar_shift, block_mask=block_mask, update_cache_slice=update_cache_slice,
                                    continuous_mode=continuous_mode, x_img_emb=x_img_emb, **kwargs)
        logits = self.backbone(x, sigma, continuous_mode=continuous_mode, x_img_emb=x_img_emb, block_mask=block_mask,
                               update_cache_slice=update_cache_slice, **kwargs)
        if return_logits:
            return logits
        if logits.requires_grad:
            raise RuntimeError("unidisc_amd.Diffusion.forward: full SUBS log-probs are an inference product (no autograd); "
                               "training uses compute_loss (fused path) — wrap sampler calls in torch.no_grad()")
        return self._subs_parameterization(logits, xt=x, batch=batch, **kwargs)

    def _ar_forward(self, x, batch, return_logits, disable_ar_shift, **kwargs):
        """model.py:717-781, AR branch: logits[:, :-1] (ar_shift), the [MASK] column excluded and - under force_argmax_valid_indices, when the modality map
        is one longer than the shifted logits - the other modality's ids than the TARGET token's, then log-softmax.  Excluded ids read -1e6 (the SUBS
        kernel's neg_infinity; the reference writes -1e6 / finfo.min before its log-softmax: their probability is 0 either way).  Inference product."""
        logits = self.backbone(x, None, **kwargs)
        shift = bool(cfg_get(cfg_get(self.config, "trainer"), "ar_shift", False)) and not disable_ar_shift
        if shift:
            logits = logits[:, :-1]
        if return_logits:
            return logits
        if logits.requires_grad:
            raise RuntimeError("unidisc_amd.Diffusion.forward: full AR log-probs are an inference product (no autograd); training uses compute_loss")
        B, Lo, V = logits.shape
        mod = kwargs.get("modality") if batch is None else batch.get("modality")
        if self._restrict() and mod is None:
            mod = self._static_modality(B, x.shape[1], x.device)
        mod = mod[:, 1:] if (self._restrict() and mod is not None and mod.shape[1] == Lo + 1) else None
        xt = torch.full((B, Lo), self.mask_index, dtype=torch.int64, device=x.device)   # every row "masked": the SUBS log-prob of such a row is the AR one
        flat = torch.zeros((B * Lo, (V + 7) // 8 * 8), dtype=torch.bfloat16, device=logits.device)
        flat[:, :V] = logits.reshape(B * Lo, V)
        out = K.subs_logprobs(flat, xt.reshape(-1), mod.reshape(-1).contiguous() if mod is not None else None, V, self.text_vocab_size, self.mask_index,
                              mod is not None, out_dtype=torch.bfloat16)
        return out.view(B, Lo, V)

    # ---- the host sampler: `Diffusion.sample` with its four predictors, classifier-free guidance (config.eval.cfg, one pass over
    # [x ; x_uncond] or two with config.eval.split_cfg_batches), eval.attention_caching, eval.conditioning_cache, the step tail, and the AR sampler
    def _sample_prior(self, *batch_dims):  # model_eval.py:1734-1735
        return self.mask_index * torch.ones(*batch_dims, dtype=torch.int64, device=self.device)

    def _static_modality(self, B, L, device):
        return static_modality(B, L, self.static_img_sl, device)

    def _row_modality(self, rows, B, L, modality):
        """Per-row modality for the SUBS vocabulary restriction (model.py:627-635), or None when it is off."""
        if not self._restrict():
            return None
        if modality is None:  # static slices
            modality = self._static_modality(B, L, rows.device)
        return modality.reshape(-1).to(torch.int64).index_select(0, rows)

    def _sigma(self, t):
        """what the backbone takes as sigma at time t"""
        sigma_t, _ = self.noise(t)
        return self._process_sigma(sigma_t)

    def _excluded_ids(self, ids, row_modality):
        """bool [1 or R, V] over ids = arange(V): the [MASK] id and, with row_modality [R] (force_argmax_valid_indices), the other modality's ids"""
        bad = (ids == self.mask_index)[None]
        if row_modality is not None:
            bad = bad | torch.where((row_modality == 1)[:, None], ids[None] < self.text_vocab_size, ids[None] >= self.text_vocab_size)
        return bad

    @staticmethod
    def _top_p_draw(probs, top_p, generator=None):
        """the shared end of both nucleus samplers: sort, keep cumsum <= top_p plus the top id, renormalise, multinomial -> id per row"""
        sp, si = torch.sort(probs, descending=True, dim=-1)
        keep = sp.cumsum(-1) <= top_p
        keep[..., 0] = True
        fp = sp * keep
        return si.gather(-1, torch.multinomial(fp / fp.sum(-1, keepdim=True), 1, generator=generator)).squeeze(-1)

    def get_cfg_weight(self, t):  # model_eval.py:1737-1758
        ev = cfg_get(self.config, "eval", None)
        c = cfg_get(ev, "cfg", None)
        lo, hi = cfg_get(ev, "cfg_min_timestep", None), cfg_get(ev, "cfg_max_timestep", None)
        if not cfg_get(ev, "force_cfg_value", False):
            if c == -1:
                c = torch.linspace(0, 10, t.shape[0]).to(t.device)
            if lo is not None and hi is not None:
                w = (c * ((t - hi) / (lo - hi)))[:, None]
            else:
                w = (c * (1 - t))[:, None]
        else:
            w = c
        if lo is not None:
            w = torch.where(t > lo, w, torch.tensor(0.0, device=t.device))
        if hi is not None:
            w = torch.where(t < hi, w, torch.tensor(0.0, device=t.device))
        return w if isinstance(w, torch.Tensor) else torch.tensor(w)

    def _pair_masked_logits(self, x, x_uncond, sigma, modality, sample_ids, plan_ids, w, split, **fwd_kw):
        """The guided pair forward (CFG branch of `_ddpm_forward`, model_eval.py:1763-1817) -> MaskedLogits: the conditional input x and the unconditional
        one x_uncond [B, L] through the backbone, the head on the [MASK] positions of `plan_ids` in both, so the two logits blocks line up row for row.
        Unsplit (:1787-1803): ONE pass over [x ; x_uncond]; `split` (:1770-1784, eval.split_cfg_batches): two passes of B rows, half the activation memory.
        w: the guidance weight per batch row ([B], or one value for all), or None - both halves still run and the record is the unguided one (the
        conditioning-cache build step).  `fwd_kw` goes to `forward_masked_logits`; with `conditioning_cache` the unconditional half lives at cache row B."""
        fwd = self.backbone.forward_masked_logits
        B, L = x.shape
        cat2 = (lambda v: None if v is None else torch.cat([v, v], 0))
        if sample_ids is not None:   # (named only where there are some: the conditioning cache's forward takes none)
            fwd_kw = dict(fwd_kw, sample_ids=sample_ids if split else cat2(sample_ids))
        if split:
            second = dict(fwd_kw, cache_row0=B) if "conditioning_cache" in fwd_kw else fwd_kw
            logits, rows, n = fwd(x, sigma, modality=modality, plan_ids=plan_ids, **fwd_kw)
            logits_u, _, n_u = fwd(x_uncond, sigma, modality=modality, plan_ids=plan_ids, **second)
            assert n_u == n
        else:
            both, rows, n2 = fwd(torch.cat([x, x_uncond], 0), cat2(sigma), modality=cat2(modality), plan_ids=cat2(plan_ids), **fwd_kw)
            n = n2 // 2   # the stable partition lists the [MASK] rows of the first half, then the same positions of the second half
            logits, logits_u = both, both[n:]
        if w is None:
            return MaskedLogits.of(logits, rows, n)
        b_of = torch.div(rows[:n], L, rounding_mode="floor")
        w_b = w.to(torch.float32).reshape(-1)
        w_rows = (w_b.index_select(0, b_of) if w_b.numel() == B else w_b.expand(B).index_select(0, b_of)).contiguous()
        return MaskedLogits(logits[:n], rows[:n], n, logits_u[:n], w_rows)

    def _uncond_input(self, x, x0_unmask):
        """x with the conditioning masked: the unconditional half of a guided forward"""
        x_uncond = x.clone()
        x_uncond[x0_unmask] = self.mask_index
        return x_uncond

    def _guided_masked_logits(self, x, t, sigma, x0_unmask, modality, sample_ids):
        """The guided MaskedLogits of the [MASK] rows of x, or None - without a forward - when there is no guidance or its weight is zero everywhere."""
        ev = cfg_get(self.config, "eval", None)
        if getattr(self, "_cond", None) is not None:   # eval.conditioning_cache: every forward of the run goes through the conditioning K / V cache
            return self._cond_masked_logits(x, t, sigma, x0_unmask)
        if cfg_get(ev, "cfg", None) is None or x0_unmask is None or not bool(x0_unmask.any()):
            return None
        w = self.get_cfg_weight(t)
        if not bool((w > 0).any()):
            return None
        return self._pair_masked_logits(x, self._uncond_input(x, x0_unmask), sigma, modality, sample_ids, x, w, bool(cfg_get(ev, "split_cfg_batches", False)))

    def _step_logits(self, x, t, x0_unmask, modality, sample_ids, **fwd_kw):
        """The MaskedLogits a sampler step draws from, at time t [B]: guided where guidance applies, else one plain forward.  `fwd_kw` (a block mask, the
        modality cache of eval.attention_caching) rules guidance out."""
        sig = self._sigma(t)
        rec = self._guided_masked_logits(x, t, sig, x0_unmask, modality, sample_ids) if not fwd_kw else None
        if rec is None:
            rec = MaskedLogits.of(*self.backbone.forward_masked_logits(x, sig, modality=modality, sample_ids=sample_ids, **fwd_kw))
        return rec

    # ---- `eval.conditioning_cache` (extension key): conditional sampling with one modality fully given.  Under the ModalityMask that blinds the given
    # modality's queries to the other one, its K / V in every block depend on its own tokens alone - constant for the whole run (and all-[MASK], so constant
    # too, in the unconditional half of guided sampling).  Step 0 runs the full sequence and fills the backbone's conditioning cache
    # (DIT.set_conditioning_cache); every later forward runs on the generated slice and attends to [cached ; fresh] keys.  Nothing is ever stale.
    def _conditioning_setup(self, x0, x0_unmask, modality, sample_ids, caching, B, L):
        name = "unidisc_amd.Diffusion.sample: eval.conditioning_cache"
        ev = cfg_get(self.config, "eval", None)
        if caching:
            raise NotImplementedError(f"{name} with eval.attention_caching - two different caches, set one")
        if self.time_conditioning:
            raise NotImplementedError(f"{name} with time_conditioning - the cached conditioning keys would depend on sigma")
        if sample_ids is not None:
            raise NotImplementedError(f"{name} with sample_ids - built for unpacked batches")
        Lt = int(cfg_get(cfg_get(self.config, "model"), "txt_length"))
        txt_given = x0_unmask is not None and 0 < Lt < L and bool(x0_unmask[:, :Lt].all())
        img_given = x0_unmask is not None and 0 < Lt < L and bool(x0_unmask[:, Lt:].all())
        if txt_given == img_given:
            raise NotImplementedError(f"{name} needs x0 / x0_unmask with exactly one of the static slices [:txt_length] / [txt_length:] fully given in every row "
                                      f"({'both are' if txt_given else 'neither is'})")
        if modality is not None and not (bool((modality[:, :Lt] == 0).all()) and bool((modality[:, Lt:] != 0).all())):
            raise NotImplementedError(f"{name} needs the text in the static slice [:txt_length] of every sample")
        guided = cfg_get(ev, "cfg", None) is not None
        self.backbone.set_conditioning_cache(B, L, self.device, given="text" if txt_given else "image", guided=guided)
        mod_rows = modality   # what the SUBS vocabulary restriction reads per row: the static slices, written out, once x is a slice
        if mod_rows is None and self._restrict():
            mod_rows = self._static_modality(B, L, self.device)
        return dict(sl=slice(Lt, L) if txt_given else slice(0, Lt), guided=guided, split=bool(cfg_get(ev, "split_cfg_batches", False)), built=False,
                    modality=modality, mod_rows=mod_rows)

    def _cond_masked_logits(self, x, t, sigma, x0_unmask):
        """The MaskedLogits (guided where a guidance weight is > 0, t = None: unguided) of a conditioning-cache forward: "build" on the full x while the cache
        is empty - with guidance always on both halves, whatever the weights, since both halves' keys are needed later - and "read" on the generated slice
        afterwards."""
        st = self._cond
        what, mod = ("read", None) if st["built"] else ("build", st["modality"])
        w = self.get_cfg_weight(t) if (st["guided"] and t is not None) else None
        if w is not None and not bool((w > 0).any()):
            w = None
        if not st["guided"] or (st["built"] and w is None):
            out = MaskedLogits.of(*self.backbone.forward_masked_logits(x, sigma, modality=mod, conditioning_cache=what))
        else:   # (split: two passes of B rows, each on its half of the cache)
            out = self._pair_masked_logits(x, self._uncond_input(x, x0_unmask), sigma, mod, None, x, w, st["split"], conditioning_cache=what)
        st["built"] = True
        return out

    @staticmethod
    def _cache_to_slice(cache, L, sl):
        """the logits cache over [B, L] -> its rows inside positions sl, re-indexed for [B, len(sl)] (the reference slices p_x0[:, sl]; a guided cache keeps
        its second half and its weights, row for row)"""
        if cache is None:
            return None
        pos = cache.rows % L
        keep = pos < sl.stop
        if sl.start > 0:
            keep = keep & (pos >= sl.start)
        rows = torch.div(cache.rows[keep], L, rounding_mode="floor") * (sl.stop - sl.start) + pos[keep]
        if sl.start > 0:
            rows = rows - sl.start
        cut = (lambda v: None if v is None else v[keep])
        return MaskedLogits(cache.logits[keep], rows, int(keep.sum()), cut(cache.logits_u), cut(cache.w_rows))

    @torch.no_grad()
    def _ddpm_caching_update(self, x, t, dt, p_x0=None, x0=None, x0_unmask=None, modality=None, sample_ids=None, u=None, seed=None, **kwargs):
        """model_eval.py:2073-2106 for the [MASK] rows only, fused (`udm_ddpm_sample_rows`): no [B, L, V] probabilities are built.
        `p_x0` is this implementation's cache: the masked rows' logits of the last forward (reused while x does not change, like the
        reference's p_x0 cache).  `u`: explicit uniforms [B, L, V] (parity runs); otherwise Philox keyed by `seed`.
        Returns (cache, x_next, nfe) like the reference."""
        if t.ndim > 1:
            t = t.squeeze(-1)
        B, L = x.shape
        nfe = 0
        if p_x0 is None:   # (a block mask / the modality cache of eval.attention_caching_read_cache go to the forward and rule guidance out)
            p_x0 = self._step_logits(x, t, x0_unmask, modality, sample_ids, **{k: kwargs[k] for k in ("block_mask", "modality_cache") if kwargs.get(k) is not None})
            nfe = 1
        x_next = x.clone()
        if p_x0.n > 0:
            rows_n = p_x0.rows
            b_of = torch.div(rows_n, L, rounding_mode="floor")
            t_rows = t.to(torch.float32).index_select(0, b_of).contiguous()
            s_rows = (t.to(torch.float32) - dt).index_select(0, b_of).contiguous()
            u_rows = u.reshape(B * L, -1).index_select(0, rows_n).contiguous() if u is not None else None
            tok = K.ddpm_sample_rows(p_x0.logits, self.vocab_size, self.text_vocab_size, self.mask_index, t=t_rows, s=s_rows,
                                     modality=self._row_modality(rows_n, B, L, modality), restrict=self._restrict(), u=u_rows,
                                     seed=_seed_or_default(seed), logits_u=p_x0.logits_u, w=p_x0.w_rows)
            x_next.view(-1).index_copy_(0, rows_n, tok)
        return p_x0, x_next, nfe

    def _ddpm_cache_step(self, x, t, dt, state=None, **kwargs):
        """`_ddpm_caching_update` as a step of `sample`: the logits cache lives in `state` and is dropped once x has changed -> (x_next, nfe)"""
        state.cache, x_next, nfe = self._ddpm_caching_update(x, t, dt, p_x0=state.cache, **kwargs)
        if self.time_conditioning or not torch.equal(x_next, x):
            state.cache = None  # the reference's `if not allclose(x_next, x) or time_conditioning: p_x0_cache = None`
        return x_next, nfe

    @staticmethod
    def _cache_to_full(saved, text_cache, L, Lt):
        """model_eval.py:2312-2323 (eval.attention_caching): the full cache saved when the state was sliced to the text takes the text slice's current cache back
        (None when either is)"""
        if saved is None or text_cache is None:
            return None
        keep = (saved.rows % L) >= Lt
        rows_t = torch.div(text_cache.rows, Lt, rounding_mode="floor") * L + text_cache.rows % Lt
        return MaskedLogits(torch.cat([saved.logits[keep], text_cache.logits], 0), torch.cat([saved.rows[keep], rows_t], 0), int(keep.sum()) + text_cache.n)

    # ---- `maskgit` predictor (model_eval.py:2964-3001 schedule, :3046-3114 update)
    @staticmethod
    def adap_sche(x, step, mask_index, mode="arccos"):
        """Per-sample unmasking schedule [B, step]: how many tokens each step reveals (model_eval.py:2964-3001)."""
        num_masked = (x == mask_index).sum(dim=-1)
        r = torch.linspace(1, 0, step)
        if mode == "root":
            val = 1 - r ** 0.5
        elif mode == "linear":
            val = 1 - r
        elif mode == "square":
            val = 1 - r ** 2
        elif mode == "cosine":
            val = torch.cos(r * math.pi * 0.5)
        elif mode == "arccos":
            val = torch.arccos(r) / (math.pi * 0.5)
        else:
            return None
        val = val.to(x.device)
        out = []
        for n in num_masked:
            sche = ((val / val.sum()) * n).round()
            sche[sche == 0] = 1
            sche[-1] += n - sche.sum()
            sche[-1] = max(sche[-1], 0)
            out.append(sche.int())
        return torch.stack(out, dim=0)

    @torch.no_grad()
    def _nucleus_draw(self, logits, logits_u, w_rows, row_modality, top_p, temperature, seed):
        """Token per [MASK] row from the nucleus-filtered SUBS distribution (`nucleus_sampling_batch`, model_eval.py:2642-2685, quirks included: the
        temperature divides probabilities, the top id always stays).  Sort / cumsum / multinomial over [rows, V] are device tensor ops in row
        chunks: the default path; with eval.fused_nucleus the step draws through `udm_nucleus_sample_rows` instead (`_maskgit_update`)."""
        V = self.vocab_size
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        gen = torch.Generator(device=logits.device).manual_seed(int(seed) + 2)
        ids = torch.arange(V, device=logits.device)
        for lo in range(0, logits.shape[0], 2048):
            z = logits[lo:lo + 2048, :V].float()
            if logits_u is not None:
                wv = w_rows[lo:lo + 2048, None]
                z = (1 + wv) * z - wv * logits_u[lo:lo + 2048, :V].float()
            bad = self._excluded_ids(ids, None if row_modality is None else row_modality[lo:lo + 2048])
            p = torch.softmax(z.masked_fill(bad, float("-inf")), dim=-1)
            out[lo:lo + 2048] = self._top_p_draw(p / temperature, top_p, gen)
        return out

    @torch.no_grad()
    def _maskgit_nucleus_update(self, x, t, dt, **kwargs):
        """`_maskgit_nucleus_update` (model_eval.py:3118-3167): the maskgit step with the token drawn from the nucleus-filtered distribution
        (config.eval.top_p / temperature); the confidence stays log p(token) under the UNfiltered distribution."""
        ev = cfg_get(self.config, "eval", None)
        return self._maskgit_update(x, t, dt, nucleus=(float(cfg_get(ev, "top_p", 0.95)), float(cfg_get(ev, "temperature", 0.9))), **kwargs)

    @torch.no_grad()
    def _maskgit_update(self, x, t, dt, schedule=None, step=None, x0=None, x0_unmask=None, modality=None, sample_ids=None, pred=None, gumbel=None, seed=None,
                        nucleus=None, tail=None, **kwargs):
        """One `maskgit` step on the [MASK] rows only: token ~ p (or the replayed `pred`) and its log-probability from the fused row kernel
        (`udm_categorical_sample_rows`), confidence = log p + r_temp * gumbel * t, each sample keeps its num_unmask most confident predictions
        (threshold = k-th largest, as the reference).  `gumbel` [B, L]: explicit noise (replay); otherwise drawn on the device."""
        B, L = x.shape
        t_col = t if t.ndim > 1 else t[:, None]
        copy_flag = x != self.mask_index
        num_unmask = torch.minimum(schedule[:, step].to(torch.int64).to(x.device), (~copy_flag).sum(dim=-1))
        if bool(torch.all(num_unmask <= 0)):
            return (x if not tail else K.reveal_rows(x, self.mask_index, **tail)), 0      # (early exit: the padding and the write-back still apply)
        r_temp = float(cfg_get(cfg_get(self.config, "eval", None), "maskgit_r_temp", 10))
        logits, rows_n, n, logits_u, w_rows = self._step_logits(x, t_col.squeeze(-1), x0_unmask, modality, sample_ids)
        given = pred.reshape(-1).index_select(0, rows_n).contiguous() if pred is not None else None
        draw_nucleus = given is None and nucleus is not None and n > 0
        base = _seed_or_default(seed)
        if draw_nucleus and self._fused_nucleus(logits):
            # eval.fused_nucleus: token and log p(token) from one launch (`udm_nucleus_sample_rows`); nucleus_sampling_batch divides the probabilities by the
            # temperature, which is the temperature-1 distribution against the budget top_p * temperature
            tok, logp = K.nucleus_sample_rows(logits, self.vocab_size, self.text_vocab_size, self.mask_index, inv_temperature=1.0,
                                              budget=nucleus[0] * nucleus[1], modality=self._row_modality(rows_n, B, L, modality), restrict=self._restrict(),
                                              seed=base + 2, logits_u=logits_u, w=w_rows)
        else:
            if draw_nucleus:
                given = self._nucleus_draw(logits, logits_u, w_rows, self._row_modality(rows_n, B, L, modality), nucleus[0], nucleus[1], base)
            tok, logp = K.categorical_sample_rows(logits, self.vocab_size, self.text_vocab_size, self.mask_index,
                                                  modality=self._row_modality(rows_n, B, L, modality), restrict=self._restrict(), given=given,
                                                  seed=base, logits_u=logits_u, w=w_rows)
        return self._maskgit_reveal(x, copy_flag, num_unmask, rows_n, tok, logp, gumbel, seed, r_temp, t_col, tail=tail)

    def _fused_nucleus(self, logits):
        """eval.fused_nucleus (extension key, default false) and a case the fused top-p kernels take: logits on the GPU, a vocabulary they hold in registers"""
        return bool(cfg_get(cfg_get(self.config, "eval", None), "fused_nucleus", False)) and K.nucleus_supported(logits, self.vocab_size)

    def _fused_reveal(self, x):
        """eval.fused_reveal (extension key, default false) and a case `udm_reveal_rows` takes: the state on the GPU, a row the kernel holds in registers"""
        return bool(cfg_get(cfg_get(self.config, "eval", None), "fused_reveal", False)) and K.reveal_supported(x)

    def _eos_padding_ids(self, caching):
        """(eos, pad) when `trainer.force_after_eos_padding` applies to this run, else None.  model_eval.py:2390: the rule is skipped under
        eval.attention_caching and when the tokenizer's EOS is its BOS.  The ids come from the tokenizer, else from the extension keys eval.eos_token_id /
        eval.pad_token_id (as `_pad_token_id`)."""
        if not bool(cfg_get(cfg_get(self.config, "trainer", None), "force_after_eos_padding", False)) or caching:
            return None
        tk, ev = self.tokenizer, cfg_get(self.config, "eval", None)
        eos, pad, bos = (getattr(tk, n, None) if tk is not None else None for n in ("eos_token_id", "pad_token_id", "bos_token_id"))
        eos = cfg_get(ev, "eos_token_id", None) if eos is None else eos
        pad = cfg_get(ev, "pad_token_id", None) if pad is None else pad
        if eos is None or pad is None:
            raise ValueError("unidisc_amd.Diffusion.sample: trainer.force_after_eos_padding needs the EOS and pad token ids: tokenizer.eos_token_id / "
                             "tokenizer.pad_token_id, or the keys eval.eos_token_id / eval.pad_token_id; "
                             f"{'neither is' if eos is None and pad is None else ('the EOS id is not' if eos is None else 'the pad id is not')} set")
        if bos is not None and int(eos) == int(bos):
            return None
        return int(eos), int(pad)

    def _pad_after_eos(self, x, eos_pad, modality):
        """model_eval.py:2390-2394 after a sampler update: every text position strictly behind a row's first EOS (searched over the whole row) that holds a
        token other than pad and [MASK] becomes pad.  Out of place, no host read (a row without EOS has its first EOS at L: nothing lies behind it)."""
        eos, pad = eos_pad
        L = x.shape[1]
        pos = torch.arange(L, device=x.device)
        first = torch.where(x == eos, pos, torch.full((), L, device=x.device)).amin(dim=-1, keepdim=True)
        to_pad = (pos > first) & (modality == 0) & (x != pad) & (x != self.mask_index)
        return torch.where(to_pad, torch.full((), pad, dtype=x.dtype, device=x.device), x)

    def _eos_modality(self, x, modality):
        """the modality map [B, L] the EOS rule reads: the given one, else the static slices written out"""
        return modality.to(torch.int64).contiguous() if modality is not None else self._static_modality(*x.shape, x.device)

    def _maskgit_reveal(self, x, copy_flag, num_unmask, rows_n, tok, logp, gumbel, seed, r_temp, t_col, tail=None):
        """the second half of a maskgit step: confidence = log p + r_temp * gumbel * t, each sample keeps its num_unmask most confident predictions.
        `tail`: eval.fused_reveal - one launch (`udm_reveal_rows`) that also pads behind the EOS and writes x0 back (the operands of sample()'s step tail)"""
        B, L = x.shape
        if tail is not None:
            return K.reveal_rows(x, self.mask_index, rows=rows_n, tok=tok, logp=logp, sched=num_unmask, t=t_col.reshape(-1).to(torch.float32).contiguous(),
                                 noise=None if gumbel is None else gumbel.to(torch.float32).contiguous(),
                                 seed=_seed_or_default(seed) + 1, r_temp=r_temp, **tail), 1
        if gumbel is None:
            g = torch.Generator(device=x.device).manual_seed(_seed_or_default(seed) + 1)
            u = torch.rand(B, L, device=x.device, generator=g).clamp_(1e-20, 1.0)
            gumbel = -torch.log(-torch.log(u))
        conf = torch.full((B * L,), float("-inf"), dtype=torch.float32, device=x.device)
        conf.index_copy_(0, rows_n, logp)
        conf = conf.view(B, L) + torch.where(copy_flag, torch.zeros((), device=x.device), r_temp * gumbel.to(torch.float32) * t_col.to(torch.float32))
        conf = torch.where(copy_flag, torch.full_like(conf, float("-inf")), conf)
        top, _ = torch.topk(conf, k=int(num_unmask.max()), dim=-1)
        thr = top.gather(-1, torch.clamp(num_unmask - 1, min=0)[:, None])
        thr = torch.where((num_unmask <= 0)[:, None], torch.full_like(thr, float("inf")), thr)
        pred_full = x.clone()
        pred_full.view(-1).index_copy_(0, rows_n, tok)
        return torch.where(conf >= thr, pred_full, x), 1

    @torch.no_grad()
    def _first_hitting_update(self, x, t, dt, schedule=None, step=None, x0=None, x0_unmask=None, modality=None, sample_ids=None, u=None, pos_u=None, seed=None,
                              tail=None, **kwargs):
        """`_first_hitting_update` (model_eval.py:3005-3043) on the [MASK] rows: token = `_sample_categorical(p_x0)` through the fused row kernel (explicit
        uniforms `u` [B, L, V] replay the reference's draw, else Philox), then the num_unmask [MASK] positions with the largest lottery values
        `pos_u` [B, L] are revealed."""
        B, L = x.shape
        t_col = t if t.ndim > 1 else t[:, None]
        copy_flag = x != self.mask_index
        logits, rows_n, n, logits_u, w_rows = self._step_logits(x, t_col.squeeze(-1), x0_unmask, modality, sample_ids)
        num_unmask = torch.minimum(schedule[:, step].to(torch.int64).to(x.device), (~copy_flag).sum(dim=-1))
        if bool(torch.all(num_unmask <= 0)):
            return (x if not tail else K.reveal_rows(x, self.mask_index, **tail)), 1
        u_rows = u.reshape(B * L, -1).index_select(0, rows_n).contiguous() if u is not None else None
        base = _seed_or_default(seed)
        tok, _ = K.categorical_sample_rows(logits, self.vocab_size, self.text_vocab_size, self.mask_index, modality=self._row_modality(rows_n, B, L, modality),
                                           restrict=self._restrict(), u=u_rows, seed=base, logits_u=logits_u, w=w_rows)
        if tail is not None:   # eval.fused_reveal: the lottery, the padding behind the EOS and the x0 write-back in one launch (`udm_reveal_rows`)
            return K.reveal_rows(x, self.mask_index, rows=rows_n, tok=tok, sched=num_unmask, noise=None if pos_u is None else pos_u.to(torch.float32).contiguous(),
                                 seed=base + 1, lottery=True, **tail), 1
        return self._first_hitting_reveal(x, copy_flag, num_unmask, rows_n, tok, pos_u, base), 1

    @staticmethod
    def _first_hitting_reveal(x, copy_flag, num_unmask, rows_n, tok, pos_u, base):
        """the second half of a first_hitting step: the num_unmask [MASK] positions with the largest lottery values take their token"""
        B, L = x.shape
        if pos_u is None:
            pos_u = torch.rand(B, L, device=x.device, generator=torch.Generator(device=x.device).manual_seed(base + 1))
        rv = torch.where(~copy_flag, pos_u.to(torch.float32), torch.full((), -1.0, device=x.device))
        _, indices = torch.sort(rv, dim=-1, descending=True)
        final = torch.arange(L, device=x.device).expand(B, L) < num_unmask[:, None]
        result = torch.zeros_like(copy_flag)
        result.scatter_(-1, indices, final)
        pred_full = x.clone()
        pred_full.view(-1).index_copy_(0, rows_n, tok)
        return torch.where(result, pred_full, x)

    # ---- AR baseline sampler: `_ar_sampler` model_eval.py:2736-2822 on the backbone's KV cache (reset_kv_cache / forward(start_pos=...))
    def _ar_bos_id(self, bos_token_id=None):
        """tokenizer.bos_token_id (model_eval.py:2742), else the `bos_token_id=` extension, else an error"""
        bos = getattr(self.tokenizer, "bos_token_id", None) if self.tokenizer is not None else None
        if bos is None:
            bos = bos_token_id
        if bos is None:
            raise ValueError("unidisc_amd.Diffusion._ar_sampler: no BOS id - the tokenizer has no bos_token_id and no bos_token_id= was given")
        return int(bos)

    @staticmethod
    def _ar_fixed_prefix(x0_unmask, L):
        """Length n0 >= 1 of the prefix that is final in every row before decoding starts: position 0 (BOS or x0) plus the common leading run of x0_unmask
        from position 1.  Those tokens are never redrawn, so prefilling them is exact; capped at L - 1 (the positions the sampler feeds)."""
        n0 = 1
        if x0_unmask is not None:
            run = x0_unmask[:, 1:].all(0).to(torch.int64).cpu()
            n0 += int(run.cumprod(0).sum())
        return min(n0, L - 1)

    # eval.ar_chunk_min_tokens when the key is unset: the smallest chunk (tokens of one _forward_chunk call) worth leaving the decode path for.  Measured
    # (scripts/bench_ar_chunked.py part (a), RESULTS.md "Chunked cached forward"; n = 2, 4, 8, ... at p = 256): one chunk forward costs about three decode
    # steps at 1.4 B with 8 rows (n = 2: 1.46 x the two steps, n = 4: 0.74 x) and about one everywhere else measured (n = 2: 0.78 - 0.96 x), so 4 is the
    # smallest measured n that wins at both row counts of both models.  n = 3 was not measured.
    AR_CHUNK_MIN_TOKENS = 4

    @staticmethod
    def _ar_given_columns(x0_unmask):
        """given[c - 1]: column c >= 1 is given in every row - the one host read of eval.ar_chunk_given, before the token loop"""
        return x0_unmask[:, 1:].all(0).cpu().tolist()

    @staticmethod
    def _ar_given_runs(given, n0, L, min_tokens):
        """eval.ar_chunk_given: where the token loop of _ar_sampler leaves the decode path.  given[c - 1]: column c (1 <= c < L) is given in EVERY row
        (x0_unmask[:, 1:].all(0), on the host); n0: the prefilled prefix (_ar_fixed_prefix).  -> {i: r}: at step i >= n0 the columns i + 1 .. i + r are a
        maximal such run behind the prefix, so the r + 1 tokens of positions i .. i + r go through one _forward_chunk at start_pos = i, and choose(i + r)
        follows.  Position L - 1 is never fed (the cache holds L - 1 slots), so a run that reaches the last column is cut at L - 2.  Runs with
        r + 1 < min_tokens stay on the decode path; a run that touches the prefix is the prefix's (n0 already counts it)."""
        given = [bool(g) for g in given]
        assert len(given) == L - 1
        runs, c = {}, n0 + 1            # (column n0 is not given in every row, or n0 = L - 1 and nothing is left)
        while c < L:
            if not given[c - 1]:
                c += 1
                continue
            a = c
            while c < L and given[c - 1]:
                c += 1
            i, r = a - 1, min(c - 1, L - 2) - (a - 1)      # the run is columns a .. c - 1
            if r >= 1 and r + 1 >= min_tokens:
                runs[i] = r
        return runs

    @staticmethod
    def _ar_decode_positions(runs, n0, n_pred):
        """the positions of the token loop that take a decode step (the others are inside a chunk of `runs`, _ar_given_runs)"""
        out, i = [], n0
        while i < n_pred:
            r = runs.get(i, 0)
            if not r:
                out.append(i)
            i += r + 1
        return out

    @staticmethod
    def _ar_nucleus(z, top_p, temperature, generator=None):
        """`nucleus_sampling` (model_eval.py:2691-2734), not the p / T quirk of nucleus_sampling_batch: softmax(z / T), sort, keep cumsum <= top_p plus the top
        id, renormalise, multinomial.  z fp32 [R, V] with excluded ids at -inf (softmax is shift-invariant: raw logits give the log-probs' distribution)."""
        return Diffusion._top_p_draw(torch.softmax(z / temperature, dim=-1), top_p, generator)

    def _ar_require_gpu(self):
        if self.device.type != "cuda":
            raise NotImplementedError("unidisc_amd.Diffusion: the AR sampler runs on the GPU only (KV-cached decoding in HIP kernels; there is no CPU path)")

    @torch.no_grad()
    def _ar_sampler(self, B, x0=None, x0_unmask=None, modality=None, noise=None, seed=None, bos_token_id=None, **kwargs):
        """Next-token sampling of the AR baseline, KV-cached: x[:, 0] = BOS, x0 / x0_unmask conditioning, the fixed prefix prefilled in one causal forward,
        then one decode step per token; token = argmax(next + Gumbel) (noise [B, L-1, V] replays a recorded draw, otherwise Philox Gumbel from `seed`), or
        the reference's nucleus_sampling with eval.top_p.  CFG (eval.cfg with x0, eval.force_cfg_value) runs [x ; where(x0_unmask, [MASK], x)] as one
        batch on one cache.  eval.ar_chunk_given (extension): a run of columns behind the prefix that is given in every row is fed through ONE chunk
        forward over the cache (DIT._forward_chunk) instead of one decode step per token (_ar_given_runs; runs shorter than eval.ar_chunk_min_tokens and
        columns given in some rows only stay on the decode path).  Returns (x [B, L], nfe) - nfe counts the argmax steps (0 with top_p, the reference's
        quirk), chunked or not.  eval.ar_decode_graph (extension): the decode step, the token choice and the advance of a device-side position are
        captured once into a graph (DIT.capture_decode_step) and every decode position is one replay; chunks stay eager.  self.ar_decode_stats counts
        what the token loop did."""
        self._ar_require_gpu()
        assert B > 0
        assert (x0 is None) == (x0_unmask is None)
        m, ev = cfg_get(self.config, "model"), cfg_get(self.config, "eval", None)
        cfg_w = cfg_get(ev, "cfg", None)
        guided = cfg_w is not None and x0 is not None
        if guided and not cfg_get(ev, "force_cfg_value", False):
            raise NotImplementedError("unidisc_amd.Diffusion._ar_sampler: eval.cfg without eval.force_cfg_value - the reference's get_cfg_weight indexes a "
                                      "Python float there, so AR guidance exists only with a constant weight (eval.force_cfg_value=true)")
        for key in ("cfg_min_timestep", "cfg_max_timestep"):
            if guided and cfg_get(ev, key, None) is not None:
                raise NotImplementedError(f"unidisc_amd.Diffusion._ar_sampler: eval.{key} with AR guidance is not built")
        top_p = cfg_get(ev, "top_p", None)
        temperature = float(cfg_get(ev, "temperature", 1.0) or 1.0)
        # eval.ar_decode_graph (extension key, default false): a replayed step can only hold launches that read the position from device memory, which
        # the tensor top-p path (a sort, a multinomial draw from a torch.Generator, a host-indexed column write) is not
        decode_graph = bool(cfg_get(ev, "ar_decode_graph", False))
        if decode_graph and top_p is not None and not (bool(cfg_get(ev, "fused_nucleus", False)) and self.vocab_size <= K.NUCLEUS_V_MAX):
            raise NotImplementedError("unidisc_amd.Diffusion._ar_sampler: eval.ar_decode_graph with the tensor top-p path (eval.top_p without "
                                      f"eval.fused_nucleus, or a vocabulary above {K.NUCLEUS_V_MAX}) - only the fused token-choice kernels read the position "
                                      "from device memory; set eval.fused_nucleus or unset eval.ar_decode_graph")
        bos = self._ar_bos_id(bos_token_id)
        L = int(cfg_get(m, "length"))
        n_pred = L - 1
        dev = self.device
        V, Vt = self.vocab_size, self.text_vocab_size
        x = torch.zeros((B, L), dtype=torch.int64, device=dev)
        x[:, 0] = bos
        if x0 is not None:
            x0 = x0.to(dev).to(torch.int64).contiguous()
            x0_unmask = x0_unmask.to(dev).bool().contiguous()
            x = torch.where(x0_unmask, x0, x)
        restrict = self._restrict()
        if modality is None and (restrict or self.backbone.modality_embed is not None or self.backbone.rope_2d):
            modality = self._static_modality(B, L, dev)
        if modality is not None:
            modality = modality.to(dev).to(torch.int64).contiguous()
        if noise is not None:
            noise = noise.to(dev).to(torch.float32).contiguous()
            if tuple(noise.shape) != (B, n_pred, V):
                raise ValueError(f"unidisc_amd.Diffusion._ar_sampler: noise must be [{B}, {n_pred}, {V}], got {tuple(noise.shape)}")
        R = 2 * B if guided else B
        bb = self.backbone
        bb.reset_kv_cache(batch_size=R, seq_len=n_pred, dtype=self.dtype, device=dev,
                          modality=torch.cat([modality, modality], 0) if (guided and modality is not None) else modality)
        kv = bb._kv
        w = torch.full((4,), float(cfg_w) if guided else 0.0, dtype=torch.float32, device=dev)
        base_seed = _seed_or_default(seed) & ((1 << 63) - 1)
        gen = torch.Generator(device=dev).manual_seed(base_seed + 3) if top_p is not None else None
        logits = kv.logits

        fused_top_p = top_p is not None and self._fused_nucleus(logits)
        chunk_given = bool(cfg_get(ev, "ar_chunk_given", False))
        if chunk_given and top_p is not None and not fused_top_p:
            bb.reset_kv_cache(set_to_none=True)
            raise NotImplementedError("unidisc_amd.Diffusion._ar_sampler: eval.ar_chunk_given with the tensor top-p path - its torch.Generator stream is "
                                      "sequential, so skipped steps would move every later draw; eval.fused_nucleus and the Gumbel paths key their draws by step")

        def choose(i):   # token of position i + 1 from kv.logits (the next-token logits of position i); writes x and kv.ids
            if fused_top_p:   # eval.fused_nucleus: nucleus_sampling (softmax(z / T) against top_p) in one launch, no tensor operators
                K.ar_nucleus_rows(logits, x, i + 1, V, Vt, self.mask_index, inv_temperature=1.0 / temperature, budget=float(top_p), step=i, modality=modality,
                                  restrict=restrict, seed=base_seed, x0=x0, x0_unmask=x0_unmask, next_ids=kv.ids,
                                  logits_u=logits[B:] if guided else None, w=w if guided else None, rows=B)
                return
            if top_p is None:
                K.ar_sample_rows(logits, x, i + 1, V, Vt, self.mask_index, step=i, modality=modality, restrict=restrict, g=noise,
                                 g_col0=i * V, seed=base_seed, x0=x0, x0_unmask=x0_unmask, next_ids=kv.ids,
                                 logits_u=logits[B:] if guided else None, w=w if guided else None, rows=B)
                return
            z = logits[:B, :V].float()
            if guided:
                z = (1 + float(cfg_w)) * z - float(cfg_w) * logits[B:2 * B, :V].float()
            z = z.masked_fill(self._excluded_ids(torch.arange(V, device=dev), modality[:, i + 1] if restrict else None), float("-inf"))
            y = self._ar_nucleus(z, float(top_p), temperature, gen)
            col = y if x0 is None else torch.where(x0_unmask[:, i + 1], x0[:, i + 1], y)
            x[:, i + 1] = col
            kv.ids[:B] = col
            if guided:
                kv.ids[B:2 * B] = torch.where(x0_unmask[:, i + 1], torch.full_like(col, self.mask_index), col)

        def choose_at():   # choose(i) with i read from kv.pos_dev by the kernel: the token choice of the captured step
            kw = dict(modality=modality, restrict=restrict, seed=base_seed, x0=x0, x0_unmask=x0_unmask, next_ids=kv.ids,
                      logits_u=logits[B:] if guided else None, w=w if guided else None, rows=B)
            if fused_top_p:
                K.ar_nucleus_rows_at(logits, x, kv.pos_dev, V, Vt, self.mask_index, inv_temperature=1.0 / temperature, budget=float(top_p), **kw)
            else:
                K.ar_sample_rows_at(logits, x, kv.pos_dev, V, Vt, self.mask_index, g=noise, **kw)

        n0 = self._ar_fixed_prefix(x0_unmask, L)
        ids0 = x[:, :n0]
        if guided:
            ids0 = torch.cat([ids0, torch.where(x0_unmask, self.mask_index, x)[:, :n0]], 0)
        mod0 = None
        if modality is not None:
            mod0 = modality[:, :n0]
            if guided:
                mod0 = torch.cat([mod0, mod0], 0)
        # eval.ar_chunk_given (extension key, default false): runs of columns given in every row go through one chunk forward over the cache instead of one
        # decode step per token.  The segmentation is fixed here, from the one host read _ar_fixed_prefix makes too; unset, `runs` is empty.
        runs = {}
        if chunk_given and x0_unmask is not None:
            min_tokens = int(cfg_get(ev, "ar_chunk_min_tokens", None) or self.AR_CHUNK_MIN_TOKENS)
            runs = self._ar_given_runs(self._ar_given_columns(x0_unmask), n0, L, max(min_tokens, 2))
        bb._prefill(ids0, mod0, last_only=True)
        choose(n0 - 1)
        stats = self.ar_decode_stats = dict(captures=0, replays=0, eager_steps=0, chunks=0)
        graph = None
        if decode_graph and self._ar_decode_positions(runs, n0, n_pred):
            # one capture per call, on this call's cache and state tensors (nothing of it outlives the call); its eager warm-up run is undone
            bb.set_decode_position(n0)
            graph = bb.capture_decode_step(choose_at)
            stats["captures"] = 1
        i = n0
        while i < n_pred:
            r = runs.get(i, 0)
            if r:   # positions i .. i + r are final in every row (x[:, i] was just chosen, the rest is given): their logits are never drawn from but the last's
                ids = x[:, i:i + r + 1]
                if guided:
                    ids = torch.cat([ids, torch.where(x0_unmask, self.mask_index, x)[:, i:i + r + 1]], 0)
                bb._forward_chunk(ids, None, i, last_only=True)      # (modality columns i .. i + r: the cache's full-length map)
                i += r
                stats["chunks"] += 1
            elif graph is not None:   # the decode step at the device's position, the token choice and position + 1: one graph launch
                graph.replay()
                stats["replays"] += 1
                i += 1
                continue
            else:
                bb._decode_step(i)
                stats["eager_steps"] += 1
            choose(i)   # (the Philox draws are keyed by the step: the steps a chunk skipped move no other draw)
            i += 1
            if r and graph is not None:
                bb.set_decode_position(i)   # a device-side fill: the replays go on behind the chunk
        graph = None   # (holds the cache's addresses: dropped before the cache)
        bb.reset_kv_cache(batch_size=R, seq_len=n_pred, dtype=self.dtype, device=dev, set_to_none=True)
        return x, (n_pred if top_p is None else 0)

    @torch.no_grad()
    def sample(self, num_steps=None, eps=1e-5, x0=None, x0_unmask=None, batch_size=None, modality=None, sample_ids=None, seed=None, noise=None,
               noise_removal=True, return_nfe=False, predictor=None, replay=None):
        """Token sampler: the `ddpm_cache` path of `_sample` (model_eval.py:2109-2455) without the decode / logging stack: prior = all [MASK]
        (x0 / x0_unmask conditioning kept fixed), timesteps = linspace(1, eps, steps + 1), one fused update per step with the logits
        cache reused while nothing changes, final arg-max of the log-probs (`noise_removal`).  Returns token ids [B, L]
        (and the number of backbone evaluations).  `noise`: optional list of uniforms [B, L, V] per step (replay of a recorded run)."""
        if self.parameterization == "ar" and bool(cfg_get(cfg_get(self.config, "eval", None), "conditioning_cache", False)):
            raise NotImplementedError("unidisc_amd.Diffusion.sample: eval.conditioning_cache with parameterization=ar - the AR sampler has its own causal KV cache")
        if self.parameterization == "ar":   # model_eval.py:2736-2822: one step per token
            self._ar_require_gpu()
            L_ar = int(cfg_get(cfg_get(self.config, "model"), "length"))
            for name, v, ok in (("sample_ids", sample_ids, sample_ids is None), ("replay", replay, replay is None),
                                ("predictor", predictor, predictor in (None, "ar")), ("num_steps", num_steps, num_steps in (None, L_ar - 1))):
                if not ok:
                    raise NotImplementedError(f"unidisc_amd.Diffusion.sample: `{name}`={v!r} with parameterization=ar - the AR sampler takes one step per token "
                                              f"(num_steps = model.length - 1 = {L_ar - 1}), no predictor choice, no replay list and no packed sample ids")
            B = x0.shape[0] if x0 is not None else int(batch_size)
            x, nfe = self._ar_sampler(B, x0=x0, x0_unmask=x0_unmask, modality=modality, noise=noise, seed=seed)
            return (x, nfe) if return_nfe else x
        assert (x0 is None) == (x0_unmask is None)
        sampling = cfg_get(self.config, "sampling", None)
        if num_steps is None:
            num_steps = int(cfg_get(sampling, "steps", 1000)) if sampling is not None else 1000
        B = x0.shape[0] if x0 is not None else int(batch_size)
        L = x0.shape[1] if x0 is not None else int(cfg_get(cfg_get(self.config, "model"), "length"))
        x = self._sample_prior(B, L)
        if x0 is not None:
            x0 = x0.to(self.device).to(torch.int64)
            x0_unmask = x0_unmask.to(self.device).bool()
            x = torch.where(x0_unmask, x0, x)
        if modality is not None:
            modality = modality.to(self.device)
        timesteps = torch.linspace(1, eps, num_steps + 1, device=self.device)
        dt = (1 - eps) / num_steps
        base_seed = _seed_or_default(seed)
        nfe = 0
        if predictor is None:
            predictor = cfg_get(sampling, "predictor", "ddpm_cache") if sampling is not None else "ddpm_cache"
        if predictor not in _PREDICTORS:
            raise NotImplementedError(f"unidisc_amd.Diffusion.sample: predictor {predictor!r} is not built (ddpm_cache, maskgit, maskgit_nucleus, first_hitting)")
        spec = _PREDICTORS[predictor]
        update = getattr(self, spec.update)
        schedule = self.adap_sche(x, num_steps, self.mask_index, spec.schedule) if spec.schedule is not None else None   # model_eval.py:2274-2290
        ev = cfg_get(self.config, "eval", None)
        self.sample_step_modes = []
        caching = self._attention_caching_setup(predictor, x0, modality, sample_ids, B, L)
        # eval.conditioning_cache (extension key, default false): step 0 on the full x fills the conditioning K / V cache, every later step and the
        # noise-removal forward run on the generated slice (the state narrowed to it; widened again at the end)
        self._cond = None
        if ev is not None and bool(cfg_get(ev, "conditioning_cache", False)):
            self._cond = self._conditioning_setup(x0, x0_unmask, modality, sample_ids, caching is not None, B, L)
        cond = self._cond
        # trainer.force_after_eos_padding (model_eval.py:2390-2394): after every update, padding behind each row's first EOS, then the x0 write-back.  With
        # eval.fused_reveal (extension key, default false) the second half of a maskgit / first_hitting step, this padding and the write-back are one launch
        # (`udm_reveal_rows`); ddpm_cache then pads and writes back through the same kernel.
        eos_pad = self._eos_padding_ids(caching is not None)
        if x0 is not None and self._fused_reveal(x):
            x0, x0_unmask = x0.contiguous(), x0_unmask.contiguous()
        st = _SamplerState(x, x0, x0_unmask, modality, self._eos_modality(x, modality) if eos_pad is not None else None)
        for i in range(num_steps):
            t = timesteps[i] * torch.ones(B, 1, device=self.device)
            if cond is not None:   # once the cache is built the sampler's state is the generated slice
                if cond["built"] and not st.narrowed:
                    st.narrow(cond["sl"], cond["mod_rows"])
                self.sample_step_modes.append("slice" if st.narrowed else "build")
            fwd_kw = self._attention_caching_step(caching, st, i, B)   # (may narrow or widen the state; {} without eval.attention_caching)
            kw = dict(x0=st.x0, x0_unmask=st.x0_unmask, modality=st.modality, sample_ids=sample_ids, seed=base_seed + 7919 * i)
            tail = None
            if spec.schedule is None:   # ddpm_cache: the logits cache in the state; `noise`: the recorded uniforms [B, L, V] per step
                kw.update(fwd_kw, state=st, u=noise[i] if noise is not None else None)
            else:   # `replay`: per step the predictor's pair of recorded draws (pred, gumbel [B, L] / u [B, L, V], pos_u [B, L]), each or None
                tail = self._tail_operands(st, eos_pad)
                kw.update(zip(spec.draws, replay[i] if replay is not None else (None, None)), schedule=schedule, step=i, tail=tail)
            st.x, n = update(st.x, t, dt, **kw)
            nfe += n
            # the step tail: fused into the update, or - ddpm_cache under the padding key - the pad-only call of the same kernel, or the tensor statements
            in_kernel = tail is not None
            if not spec.fuses_tail and eos_pad is not None:
                tail = self._tail_operands(st, eos_pad)
                if tail is not None:
                    st.x, in_kernel = K.reveal_rows(st.x, self.mask_index, **tail), True
            if not in_kernel and (eos_pad is not None or spec.writes_back):
                st.x = self._tensor_tail(st, eos_pad)
        if caching is not None:
            if st.narrowed:   # model_eval.py:2425-2440
                st.widen()
            self.backbone.reset_kv_cache()
        if cond is not None and cond["built"] and not st.narrowed:
            st.narrow(cond["sl"], cond["mod_rows"])
        if noise_removal:  # x = forward(x, sigma(t_last)).argmax(-1): unmasked positions keep their token, masked ones take the best valid id
            sig = self._sigma(timesteps[-1] * torch.ones(B, device=self.device))
            if cond is not None:   # (unguided, like the line below: the conditional half of the cache alone)
                rec = self._cond_masked_logits(st.x, None, sig, st.x0_unmask)
            else:
                rec = MaskedLogits.of(*self.backbone.forward_masked_logits(st.x, sig, modality=st.modality, sample_ids=sample_ids))
            nfe += 1
            if rec.n > 0:
                tok = K.ddpm_sample_rows(rec.logits, self.vocab_size, self.text_vocab_size, self.mask_index,
                                         modality=self._row_modality(rec.rows, B, st.x.shape[1], st.modality), restrict=self._restrict(), greedy=True)
                st.x = st.x.clone()
                st.x.view(-1).index_copy_(0, rec.rows, tok)
            if st.x0 is not None:
                st.x = torch.where(st.x0_unmask, st.x0, st.x)
        if cond is not None:
            if st.narrowed:   # the full tensors take the generated slice back
                st.widen()
            self._cond = None
            self.backbone.reset_kv_cache()
        return (st.x, nfe) if return_nfe else st.x

    def _attention_caching_setup(self, predictor, x0, modality, sample_ids, B, L):
        """eval.attention_caching (model_eval.py:2296-2366): every `ratio` steps a full joint update, the step after it a full update in which image queries
        see image keys only, every other step on the text slice alone (the state narrowed to static_txt_sl).  Returns None when the key is off, else
        dict(ratio, Lt, read_cache) with the backbone's cache set.
        eval.attention_caching_read_cache (extension key, default false: the reference's behaviour above): the build step also fills a per-block K / V cache
        with every position's keys, and the text steps attend to [fresh text keys ; cached image keys] instead of the text keys alone - what the reference's
        comment at models/dit.py:790-792 intends.  The cached image keys are those of the x that ENTERED the last build step; they are not refreshed by the
        tokens that step or the next full step draw (the next build step does that)."""
        ev = cfg_get(self.config, "eval", None)
        if ev is None or not bool(cfg_get(ev, "attention_caching", False)):
            return None
        if predictor != "ddpm_cache" or x0 is not None or cfg_get(ev, "cfg", None) is not None or sample_ids is not None:
            raise NotImplementedError("unidisc_amd.Diffusion.sample: eval.attention_caching is built for the unconditional ddpm_cache predictor only")
        Lt = int(cfg_get(cfg_get(self.config, "model"), "txt_length"))
        read_cache = bool(cfg_get(ev, "attention_caching_read_cache", False))
        if read_cache:
            if self.time_conditioning:
                raise NotImplementedError("unidisc_amd.Diffusion.sample: eval.attention_caching_read_cache with time_conditioning - the cached image keys "
                                          "would depend on sigma")
            if modality is not None and not (bool((modality[:, :Lt] == 0).all()) and bool((modality[:, Lt:] != 0).all())):
                raise NotImplementedError("unidisc_amd.Diffusion.sample: eval.attention_caching_read_cache needs the text in the static slice [:txt_length] "
                                          "of every sample")
        self.backbone.set_flex_attention_cache(B, L, self.device, None, read_cache=read_cache)
        return dict(ratio=int(cfg_get(ev, "attention_caching_txt_to_img_ratio", 10)), Lt=Lt, read_cache=read_cache)

    def _attention_caching_step(self, caching, st, i, B):
        """Step i of eval.attention_caching: puts the state into the step's view, notes the mode in `sample_step_modes` and returns the forward's extra
        keywords (the build step's block mask, the modality cache's "build" / "read")."""
        if caching is None:
            return {}
        ratio, Lt, read_cache = caching["ratio"], caching["Lt"], caching["read_cache"]
        if i % ratio == 0:
            if st.narrowed:   # the saved full tensors take the text slice back
                st.widen(keep_cache=True)
            self.sample_step_modes.append("full")
            return {}
        if (i - 1) % ratio == 0:
            self.sample_step_modes.append("build")
            if read_cache:   # the step must run its forward (a reused logits cache would leave the K / V cache unbuilt or stale)
                st.cache = None
            block_mask = ModalityMask(torch.zeros(B, dtype=torch.bool, device=self.device), torch.ones(B, dtype=torch.bool, device=self.device), Lt)
            return dict(block_mask=block_mask, modality_cache="build") if read_cache else dict(block_mask=block_mask)
        if not st.narrowed:
            st.narrow(slice(0, Lt), st.modality)
        self.sample_step_modes.append("text")
        return dict(modality_cache="read") if read_cache else {}

    def _tail_operands(self, st, eos_pad):
        """the operands of the step tail for `udm_reveal_rows` (eval.fused_reveal), or None on the tensor path"""
        if not self._fused_reveal(st.x):
            return None
        ops = dict(eos_id=eos_pad[0], pad_id=eos_pad[1], modality=st.eos_mod) if eos_pad is not None else {}
        return dict(ops, x0=st.x0, x0_unmask=st.x0_unmask) if st.x0 is not None else ops

    def _tensor_tail(self, st, eos_pad):
        """the step tail as tensor statements: the padding behind the EOS, then the x0 write-back"""
        x = self._pad_after_eos(st.x, eos_pad, st.eos_mod) if eos_pad is not None else st.x
        return torch.where(st.x0_unmask, st.x0, x) if st.x0 is not None else x

    # ---- model.py:797-1173, SUBS / continuous-time branch
    def compute_loss(self, batch, prefix, batch_idx=-1):
        if self.parameterization == "ar":
            return self._compute_loss_ar(batch, prefix)
        cfg, tr = self.config, cfg_get(self.config, "trainer")
        kwargs = self.get_cond_dict(batch)
        modality_mask = batch.get("modality_mask", None)
        x0, attention_mask = batch["input_ids"], batch.get("attention_mask", None)
        if x0.shape[1] > cfg_get(cfg_get(cfg, "model"), "length"):
            raise NotImplementedError("unidisc_amd: sequence sub-sampling (text8-crop) is not on the denoising hot path")
        if (isinstance(self.noise, LogLinearNoise) and cfg_get(tr, "joint_ar_nar_timestep_warmup_steps", None) is None
                and cfg_get(tr, "force_timestep", None) is None):
            # `_sample_t` + the schedule + the move chance: seventeen statements on [B] tensors as one launch, bit-identical (tests/test_gpu_kernels.py); the draw stays here
            t, sigma, dsigma, mc = K.sample_t_noise(self._rand(x0.shape[0], device=x0.device).float(), antithetic=bool(self.antithetic_sampling),
                                                    sampling_eps=self.sampling_eps, noise_eps=self.noise.eps)
            move_chance = mc[:, None]
        else:
            t = self._sample_t(x0.shape[0], x0.device)
            sigma, dsigma = self.noise(t)
            move_chance = 1 - torch.exp(-sigma[:, None])
        unet_conditioning = sigma[:, None]
        xt, ignore_batch_mask_for_metrics, joint_ar_nar_mask, should_mask_txt, should_mask_img, move_indices = self.q_xt(
            x0, move_chance, return_ignore_batch_mask_for_metrics=True, batch=batch)
        m = cfg_get(cfg, "model")
        p_txt, p_img = cfg_get(m, "flex_attention_txt_masking_prob", None), cfg_get(m, "flex_attention_img_masking_prob", None)
        if (p_img is not None or p_txt is not None) and self.backbone.training:
            # modality attention dropout (model.py:863-878): per sample, text queries are restricted to text keys and / or image queries to image keys
            if p_img is None or p_txt is None:
                raise ValueError("unidisc_amd: set both model.flex_attention_txt_masking_prob and flex_attention_img_masking_prob (the reference compares both)")
            assert xt.shape[1] == cfg_get(m, "img_length") + cfg_get(m, "txt_length")
            txt_drop = self._rand(xt.shape[0], device=xt.device) < p_txt
            img_drop = self._rand(xt.shape[0], device=xt.device) < p_img
            if should_mask_txt is not None:   # a modality that is masked out entirely must not be left seeing only itself
                txt_drop = txt_drop & ~should_mask_txt.squeeze(-1)
                img_drop = img_drop & ~should_mask_img.squeeze(-1)
            kwargs["block_mask"] = ModalityMask(txt_drop, img_drop, cfg_get(m, "txt_length"))
            drop_any = (txt_drop | img_drop).unsqueeze(-1)
            ignore_batch_mask_for_metrics = drop_any if ignore_batch_mask_for_metrics is None else (ignore_batch_mask_for_metrics | drop_any)
        if cfg_get(tr, "interleaved_training_flex_attention", False):
            kwargs["sample_ids"] = batch["sample_ids"]  # the document mask is derived from sample_ids inside the attention kernel

        # fused backbone + SUBS + gather: log p_theta(x0 | xt) per token, fp32 (model.py:908-925, :967)
        log_p_theta = self.backbone.forward_logp(xt, x0, self._process_sigma(unet_conditioning), modality=kwargs.get("modality"),
                                                 sample_ids=kwargs.get("sample_ids"), restrict_modality=self._restrict(),
                                                 block_mask=kwargs.get("block_mask"), attention_mask=kwargs.get("attention_mask"))
        self._flush_checks()   # (the forward has already waited for this step's [MASK]-row count: the queued batch checks are complete, no extra wait)
        self._last = dict(t=t, sigma=sigma, dsigma=dsigma, xt=xt, move_indices=move_indices, log_p_theta=log_p_theta, modality=kwargs.get("modality"))

        # The loss arithmetic of model.py:1010-1160 (schedule weights, masked mean or the modality-weighted text / image sum with the optional text-loss cap,
        # the reported per-token NLLs and fractions) runs as ONE launch - K.diffusion_loss - instead of ~75 small tensor statements between the forward and
        # the backward; the differentiable loss is that launch's value with d loss / d log_p = its coefficient tensor (the loss is linear in log_p).
        if cfg_get(tr, "no_ce_weighting", False):
            w_std = torch.ones_like(sigma)
            w_loss = w_std
        else:
            w_std = dsigma / torch.expm1(sigma)
            gamma = cfg_get(tr, "softmin_snr", None)
            w_loss = dsigma / (torch.expm1(sigma) + (1 / gamma)) if gamma is not None else w_std
        weighted = cfg_get(tr, "text_loss_weight", None) is not None and cfg_get(tr, "img_loss_weight", None) is not None
        use_mm = (cfg_get(tr, "multimodal_batches", False) or weighted) and modality_mask is not None
        if weighted and modality_mask is None:
            raise ValueError("unidisc_amd: trainer.text_loss_weight / img_loss_weight need batches with a modality map")
        std_nlls, coef, sc = K.diffusion_loss(
            log_p_theta.detach().float(), w_loss.float(), w_std.float(), attention_mask, modality_mask if use_mm else None, weighted=weighted,
            full_mask=bool(cfg_get(tr, "force_full_attention_mask_loss_only", False)),
            text_w=float(cfg_get(tr, "text_loss_weight", None)) if weighted else 1.0,   # an explicit 0.0 stays 0.0 (model.py:1041-1044 multiplies by the configured value)
            img_w=float(cfg_get(tr, "img_loss_weight", None)) if weighted else 1.0, ratio=cfg_get(tr, "set_max_txt_loss_ratio", None) if weighted else None)
        loss = _LinearLoss.apply(log_p_theta, coef, sc[0])
        loss_dict = dict(loss=loss, extra_losses=dict())
        if cfg_get(tr, "log_seperate_modal_losses", False):
            loss_dict.update(dict(std_txt_loss=std_nlls * modality_mask[..., 0], std_img_loss=std_nlls * modality_mask[..., 1]))
        if cfg_get(tr, "mask_entire_modality", None) is not None and self.backbone.training:
            loss_dict["batch_ignore_loss"] = ignore_batch_mask_for_metrics.reshape(-1)  # (reference: .squeeze(-1), which breaks its own interleaved branch at B = 1)
        if use_mm:
            loss_dict["extra_losses"]["trainer/img_frac"] = sc[4]
            loss_dict["extra_losses"]["trainer/txt_frac"] = sc[3]
            loss_dict["extra_losses"]["trainer/attention_mask_valid_frac"] = sc[5]
            if "batch_ignore_loss" in loss_dict:
                loss_dict["extra_losses"]["trainer/ignore_batch_metrics_frac"] = loss_dict["batch_ignore_loss"].sum() / loss_dict["batch_ignore_loss"].numel()
        if weighted:
            loss_dict.update(dict(txt_loss=sc[1], img_loss=sc[2]))
        if "batch_ignore_loss" in loss_dict:
            attention_mask = torch.where(loss_dict["batch_ignore_loss"][:, None].repeat(1, attention_mask.shape[-1]),
                                         torch.full_like(attention_mask, False), attention_mask)
        losses = Loss(loss=loss_dict["loss"], img_loss=loss_dict.get("img_loss", 0), txt_loss=loss_dict.get("txt_loss", 0), nlls=std_nlls,
                      txt_nlls=loss_dict.get("std_txt_loss", 0), img_nlls=loss_dict.get("std_img_loss", 0), token_mask=attention_mask,
                      modality_mask=modality_mask, extra_losses=loss_dict.get("extra_losses", None))
        return self._finish_loss(losses, prefix)

    def _compute_loss_ar(self, batch, prefix):
        """model.py:840-1073 for parameterization=ar with trainer.ar_shift: x_t = x_0 (no t draw, no corruption), sigma = None, next-token log-probs from the
        causal backbone's shifted head (DIT.forward_logp(ar_shift=True): the fused SUBS cross-entropy with every row "masked"), weight 1, and the reference's
        reductions over the SHIFTED attention mask / modality mask (masked mean, or the text / image-weighted form) in one K.diffusion_loss launch."""
        cfg, tr = self.config, cfg_get(self.config, "trainer")
        kwargs = self.get_cond_dict(batch)
        if "attention_mask" in kwargs:
            raise NotImplementedError("unidisc_amd: parameterization=ar with model.use_attention_mask - an attention mask beside is_causal is an SDPA error in the reference")
        x0, attention_mask, modality_mask = batch["input_ids"], batch.get("attention_mask", None), batch.get("modality_mask", None)
        if x0.shape[1] > cfg_get(cfg_get(cfg, "model"), "length"):
            raise NotImplementedError("unidisc_amd: sequence sub-sampling (text8-crop) is not on the denoising hot path")
        log_p_full = self.backbone.forward_logp(x0, x0, self._process_sigma(None), modality=kwargs.get("modality"), restrict_modality=self._restrict(),
                                                ar_shift=True)
        self._flush_checks()
        log_p_theta = log_p_full[:, :-1]   # (the last column has no target: 0, zero gradient)
        attention_mask = attention_mask[:, 1:]
        if modality_mask is not None:
            modality_mask = modality_mask[:, 1:]
        self._last = dict(t=None, sigma=None, dsigma=None, xt=x0, move_indices=None, log_p_theta=log_p_theta, modality=kwargs.get("modality"))
        ones = torch.ones(x0.shape[0], dtype=torch.float32, device=x0.device)   # std_weighting = 1 (model.py:972-975), no soft-min SNR
        weighted = cfg_get(tr, "text_loss_weight", None) is not None and cfg_get(tr, "img_loss_weight", None) is not None
        use_mm = (cfg_get(tr, "multimodal_batches", False) or weighted) and modality_mask is not None
        if weighted and modality_mask is None:
            raise ValueError("unidisc_amd: trainer.text_loss_weight / img_loss_weight need batches with a modality map")
        std_nlls, coef, sc = K.diffusion_loss(
            log_p_theta.detach().float().contiguous(), ones, ones, attention_mask.contiguous(), modality_mask.contiguous() if use_mm else None, weighted=weighted,
            full_mask=bool(cfg_get(tr, "force_full_attention_mask_loss_only", False)),
            text_w=float(cfg_get(tr, "text_loss_weight", None)) if weighted else 1.0,
            img_w=float(cfg_get(tr, "img_loss_weight", None)) if weighted else 1.0, ratio=cfg_get(tr, "set_max_txt_loss_ratio", None) if weighted else None)
        loss = _LinearLoss.apply(log_p_theta, coef, sc[0])
        extra = dict()
        if use_mm:
            extra["trainer/img_frac"], extra["trainer/txt_frac"], extra["trainer/attention_mask_valid_frac"] = sc[4], sc[3], sc[5]
        sep = cfg_get(tr, "log_seperate_modal_losses", False)
        losses = Loss(loss=loss, img_loss=sc[2] if weighted else 0, txt_loss=sc[1] if weighted else 0, nlls=std_nlls,
                      txt_nlls=std_nlls * modality_mask[..., 0] if sep else 0, img_nlls=std_nlls * modality_mask[..., 1] if sep else 0,
                      token_mask=attention_mask, modality_mask=modality_mask, extra_losses=extra)
        return self._finish_loss(losses, prefix)

    def _finish_loss(self, losses, prefix):
        tr = cfg_get(self.config, "trainer")
        if cfg_get(tr, "disable_torchmetrics", False):
            raise NotImplementedError("Torchmetrics disabled")
        if prefix == "train":
            return losses
        # model.py:1163-1171: validation / test update the metric collections the trainer attached (any object with .update(values, mask))
        if prefix == "val":
            if getattr(self, "valid_metrics", None) is None:
                raise RuntimeError("unidisc_amd.compute_loss(prefix='val'): attach `valid_metrics` (and optionally `valid_txt_metrics` / `valid_img_metrics`) first")
            self.valid_metrics.update(losses.nlls, losses.token_mask)
            if getattr(self, "valid_txt_metrics", None) is not None:
                self.valid_txt_metrics.update(losses.txt_nlls, losses.modality_mask[..., 0] & losses.token_mask)
                self.valid_img_metrics.update(losses.img_nlls, losses.modality_mask[..., 1] & losses.token_mask)
            return None
        if prefix == "test":
            if getattr(self, "test_metrics", None) is None:
                raise RuntimeError("unidisc_amd.compute_loss(prefix='test'): attach `test_metrics` first")
            self.test_metrics.update(losses.nlls, losses.token_mask)
            return None
        raise ValueError(f"Invalid prefix: {prefix}")

    # ---- zero-shot likelihood scoring (model_eval.py:263-652, :3569-3609): the diffusion ELBO of an (image, text) pair as a match score, and the retrieval /
    # Winoground accuracies built on it.  Under SUBS a position that is not [MASK] in x_t has log p(x0) = 0 (model.py:646-656), so per timestep only the rows
    # with x_t = [MASK] that are not padding and (unless do_unconditional) not conditioning contribute: the backbone's head runs on exactly those rows
    # (`forward_masked_logits(plan_ids=...)`), `udm_subs_logp_rows` turns their logits - both halves of a guided pass, mixed in fp32 - into log p(x0), and
    # `udm_likelihood_scores` sums them per sample.  No [B, L, V] tensor is built.
    def _pad_token_id(self):
        pad = getattr(self.tokenizer, "pad_token_id", None) if self.tokenizer is not None else None
        if pad is None:
            pad = cfg_get(cfg_get(self.config, "eval", None), "pad_token_id", None)
        if pad is None:
            raise ValueError("unidisc_amd.get_similarity: the pad token id comes from tokenizer.pad_token_id or eval.pad_token_id; neither is set")
        return int(pad)

    def _similarity_refusals(self, batch, what):
        m = cfg_get(self.config, "model")
        if self.time_conditioning or cfg_get(m, "force_time_conditioning", False):
            raise NotImplementedError(f"unidisc_amd.{what}: time_conditioning - the reference scores with sigma = None (model_eval.py:316), a time-conditioned "
                                      "backbone has no such input")
        if cfg_get(m, "img_first", False):
            raise NotImplementedError(f"unidisc_amd.{what}: model.img_first - the [image, text] layout of the scoring branches (model_eval.py:580-627) is not built")
        if batch is not None and batch.get("sample_ids") is not None:
            raise NotImplementedError(f"unidisc_amd.{what}: packed sample_ids - the score assumes one (text, image) pair per row (model_eval.py:269)")

    def _similarity_cfg_weight(self, t):
        """`cfg` (model_eval.py:2630-2640): w = eval.cfg (1 - t) per sample, linspace(0, 10, B) (1 - t) for eval.cfg = -1, the scalar itself under
        eval.force_cfg_value.  NOT get_cfg_weight: no cfg_min / cfg_max_timestep windows here."""
        ev = cfg_get(self.config, "eval", None)
        c = cfg_get(ev, "cfg", None)
        if cfg_get(ev, "force_cfg_value", False):
            return torch.full_like(t, float(c), dtype=torch.float32)
        if c == -1:
            c = torch.linspace(0, 10, t.shape[0]).to(t.device)
        return (c * (1 - t)).to(torch.float32)

    def _similarity_times(self, num_timesteps, B, device, randomize):
        """model_eval.py:277-287: the interior points of linspace(0, 1, T + 2), or sorted uniforms - one set for the batch, or one per sample ([B, T])."""
        ev = cfg_get(self.config, "eval", None)
        times = torch.linspace(0, 1, steps=num_timesteps + 2)[1:-1].to(device).to(torch.float32)
        if randomize and cfg_get(ev, "use_random_timesteps_same_batch", False):
            times = torch.sort(self._rand(num_timesteps, device=device))[0]
        if randomize and cfg_get(ev, "use_random_timesteps_diff_batch", False):
            times = torch.sort(self._rand(B, num_timesteps, device=device))[0]
        return times

    @torch.no_grad()
    def _likelihood_scores(self, x0, batch, times, valid, cond_mask, do_unconditional, guided, qxt_batch):
        """The timestep loop shared by get_similarity and get_model_likelihood_score -> (weighted [T, B], unweighed [T, B]).
        valid [B, L]: the positions that count (non-pad / attention mask); cond_mask [B, L] or None: the conditioning columns.
        One `rand(B, L)` draw per timestep in ascending order (q_xt), whatever `eval.similarity_timesteps_per_pass` (k) is: k consecutive timesteps are
        corrupted one by one and then stacked into one backbone pass of k B rows.  Nothing in the loop reads a device value on the host except the row count
        that `forward_masked_logits` itself waits for (counted on a side stream while the blocks are queued)."""
        ev = cfg_get(self.config, "eval", None)
        B, L = x0.shape
        T = times.shape[-1]
        k = max(1, int(cfg_get(ev, "similarity_timesteps_per_pass", 1) or 1))
        modality = batch["modality"]
        mask_id = self.mask_index
        other_id = (mask_id + 1) % self.vocab_size            # any id but [MASK]: marks the rows of plan_ids that need no logits
        count = valid.sum(dim=-1).to(torch.float32)
        full_mask = torch.full_like(x0, mask_id)
        split = bool(cfg_get(ev, "split_cfg_batches", False))
        out_w, out_u = [], []
        record = getattr(self, "_similarity_trace", None)   # tests: a list that receives every timestep's t, x_t, model inputs, row selection and weights
        for i0 in range(0, T, k):
            steps = range(i0, min(i0 + k, T))
            conds, unconds, plans, wstds, ws = [], [], [], [], []
            for i in steps:
                t = times[:, i] if times.dim() == 2 else times[i].expand(B)
                sigma, dsigma = self.noise(t)
                move_chance = 1 - torch.exp(-sigma[:, None])
                xt = self.q_xt(x0, move_chance, batch=qxt_batch)
                contributes = (xt == mask_id) & valid
                if cond_mask is not None and not do_unconditional:
                    contributes = contributes & ~cond_mask
                conds.append(xt if (do_unconditional or cond_mask is None) else torch.where(cond_mask, x0, xt))
                plans.append(torch.where(contributes, full_mask, torch.full_like(x0, other_id)))
                wstds.append((dsigma / torch.expm1(sigma)).to(torch.float32))
                if guided:
                    unconds.append(torch.where(cond_mask, full_mask, xt))
                    ws.append(self._similarity_cfg_weight(t))
                if record is not None:
                    record.append(dict(t=t, xt=xt, cond=conds[-1], uncond=unconds[-1] if guided else None, contributes=contributes,
                                       w=ws[-1] if guided else None))
            kk = len(conds)
            cond, plan = torch.cat(conds, 0), torch.cat(plans, 0)
            mod_k = modality.repeat(kk, 1) if modality is not None else None
            if guided:   # the pair forward of the samplers, the weights of the k B rows one per row
                logits, rows_n, n, logits_u, w_rows = self._pair_masked_logits(cond, torch.cat(unconds, 0), None, mod_k, None, plan, torch.cat(ws, 0), split)
            else:
                logits, rows_n, n, logits_u, w_rows = MaskedLogits.of(*self.backbone.forward_masked_logits(cond, None, modality=mod_k, plan_ids=plan))
            x0_rows = x0.repeat(kk, 1).reshape(-1).index_select(0, rows_n)
            log_p = K.subs_logp_rows(logits, x0_rows, self._row_modality(rows_n, kk * B, L, mod_k), self.vocab_size, self.text_vocab_size, mask_id,
                                     self._restrict(), logits_u=logits_u, w=w_rows)
            weighted, unweighed = K.likelihood_scores(log_p, rows_n, torch.cat(wstds, 0).contiguous(), count.repeat(kk).contiguous(), L)
            out_w.append(weighted.view(kk, B))
            out_u.append(unweighed.view(kk, B))
        return torch.cat(out_w, 0), torch.cat(out_u, 0)

    @torch.no_grad()
    def get_similarity(self, x0, batch, num_timesteps=None, txt_cond=True, return_unweighed=False, do_unconditional=False):
        """model_eval.py:268-378 (nested in `zero_shot_eval_step` there): the score [B] of every row of x0 = [text ; image] - the mean over `num_timesteps`
        of sum_l(-log p(x0_l | x_t) dsigma / expm1(sigma)) / #non-pad (or without the weight: `return_unweighed` / eval.return_unweighed_sim) over the positions
        that are not padding and not conditioned on (text conditions when `txt_cond`, the image otherwise; `do_unconditional`: nothing does).  Lower = better
        match.  With eval.cfg the logits are z = (1 + w) l_cond - w l_uncond (`cfg` :2630-2640).  A row without non-pad tokens scores NaN, as there."""
        if self.parameterization == "ar":
            raise ValueError("unidisc_amd.get_similarity is the diffusion score; parameterization=ar uses get_similarity_ar")
        self._similarity_refusals(batch, "get_similarity")
        ev = cfg_get(self.config, "eval", None)
        m = cfg_get(self.config, "model")
        return_unweighed = return_unweighed or bool(cfg_get(ev, "return_unweighed_sim", False))
        num_timesteps = num_timesteps or cfg_get(cfg_get(self.config, "sampling", None), "steps", None)
        if not num_timesteps:
            raise ValueError("unidisc_amd.get_similarity: num_timesteps is not given and sampling.steps is not set")
        B = batch["modality"].shape[0]
        times = self._similarity_times(int(num_timesteps), B, x0.device, randomize=True)
        do_unconditional = do_unconditional or bool(cfg_get(ev, "do_unconditional", False))
        cond_mask = torch.zeros_like(x0, dtype=torch.bool)
        if txt_cond:
            cond_mask[:, :cfg_get(m, "txt_length")] = True
        else:
            cond_mask[:, cfg_get(m, "txt_length"):] = True
        valid = x0 != self._pad_token_id()
        weighted, unweighed = self._likelihood_scores(x0, batch, times, valid, cond_mask, do_unconditional, cfg_get(ev, "cfg", None) is not None, batch)
        return (unweighed if return_unweighed else weighted).mean(dim=0)

    @torch.no_grad()
    def get_model_likelihood_score(self, batch, num_timesteps=100, return_unweighed=True):
        """model_eval.py:3569-3609: the unconditional form on batch['input_ids'] - every position of batch['attention_mask'] counts, no guidance."""
        if self.parameterization == "ar":
            raise ValueError("unidisc_amd.get_model_likelihood_score is the diffusion score (parameterization=subs)")
        self._similarity_refusals(batch, "get_model_likelihood_score")
        x0 = batch["input_ids"]
        times = self._similarity_times(int(num_timesteps), x0.shape[0], x0.device, randomize=False)
        weighted, unweighed = self._likelihood_scores(x0, batch, times, batch["attention_mask"].bool(), None, True, False, None)
        return (unweighed if return_unweighed else weighted).mean(dim=0)

    @torch.no_grad()
    def get_similarity_ar(self, x0, batch, txt_cond=True, do_unconditional=False, **kwargs):
        """model_eval.py:380-422 (AR baseline): mean next-token NLL over the non-pad positions of the whole row (`do_unconditional`), of the image part
        (`txt_cond`) or of the text part.  Runs on `Diffusion.forward`."""
        if kwargs.get("img_first", False):
            raise NotImplementedError("unidisc_amd.get_similarity_ar: img_first - the [image, text] order (model_eval.py:383-386) is not built")
        ev = cfg_get(self.config, "eval", None)
        Lt = cfg_get(cfg_get(self.config, "model"), "txt_length")
        do_unconditional = do_unconditional or bool(cfg_get(ev, "do_unconditional", False))
        mod = batch["modality"]
        model_output = self.forward(x=x0, sigma=None, modality=mod)        # eval.cfg is not applied to AR scores (:392-393)
        x0 = x0[:, 1:]
        attention_mask = x0 != self._pad_token_id()
        log_p_theta = model_output.float().gather(-1, x0[:, :, None])[:, :, 0]
        txt_sl, img_sl = slice(None, Lt - 1), slice(Lt - 1, None)
        nll = (-log_p_theta * attention_mask).sum(dim=-1) / attention_mask.sum(dim=-1)
        txt_nll = (-log_p_theta[:, txt_sl] * attention_mask[:, txt_sl]).sum(dim=-1) / attention_mask[:, txt_sl].sum(dim=-1)
        img_nll = (-log_p_theta[:, img_sl] * attention_mask[:, img_sl]).sum(dim=-1) / attention_mask[:, img_sl].sum(dim=-1)
        if do_unconditional:
            return nll
        return img_nll if txt_cond else txt_nll

    def _zero_shot_update(self, name, value):
        """running means as plain sums on the object (the reference keeps torchmetrics objects: model_setup.py:241-246)"""
        acc = self.__dict__.setdefault("zero_shot_metrics", {})
        s, n = acc.get(name, (0.0, 0))
        acc[name] = (s + float(value), n + 1)

    def zero_shot_metric(self, name):
        s, n = self.__dict__.get("zero_shot_metrics", {}).get(name, (0.0, 0))
        return s / n if n else float("nan")

    @torch.no_grad()
    def zero_shot_eval_step(self, batch, batch_idx):
        """model_eval.py:263-652, the token-level branches: Winoground-style (data.train = "facebook/winoground": the four token tensors
        input_ids_{0,1}_{0,1} = caption i with image j are given in the batch) and DataComp-style retrieval (anything else) in both eval.only_one_correct
        forms.  Returns the dict of this batch's accuracies (and per-row flags); the running means are `zero_shot_metric(name)`."""
        ev = cfg_get(self.config, "eval", None)
        m = cfg_get(self.config, "model")
        dataset_name = cfg_get(cfg_get(self.config, "data"), "train", None)
        if cfg_get(ev, "wino_chameleon", False):
            raise NotImplementedError("unidisc_amd.zero_shot_eval_step: eval.wino_chameleon - scoring with a Chameleon model (model_eval.py:424-466) is outside this project")
        if dataset_name == "nlphuji/flickr30k":
            raise NotImplementedError("unidisc_amd.zero_shot_eval_step: the flickr30k captioning / CIDEr branch (model_eval.py:468-478) needs a VAE and a text decoder")
        self._similarity_refusals(batch, "zero_shot_eval_step")
        if "modality_mask" not in batch:   # zero_shot_update_batch, model.py:154
            batch = dict(batch, modality_mask=F.one_hot(batch["modality"], num_classes=2).to(torch.bool))
        ar = self.parameterization == "ar"
        Lt = cfg_get(m, "txt_length")
        if dataset_name == "facebook/winoground":
            a = {(i, j): batch[f"input_ids_{i}_{j}"] for i in (0, 1) for j in (0, 1)}
            results_cond, out = {}, {}
            for mode in ("image", "text", "group"):
                do_unconditional = mode == "group"
                txt_cond = mode != "text"
                if ar:
                    if mode == "text":
                        raise NotImplementedError("unidisc_amd.zero_shot_eval_step: the AR text mode scores img_first sequences (model_eval.py:519), which is not built")
                    s = {ij: self.get_similarity_ar(x, batch, txt_cond=False, do_unconditional=do_unconditional) for ij, x in a.items()}
                else:
                    s = {ij: self.get_similarity(x, batch, txt_cond=txt_cond, do_unconditional=do_unconditional) for ij, x in a.items()}
                # s[(i, j)]: caption i with image j; lower is better (:506-514)
                text_ok = torch.logical_and(s[0, 0] < s[1, 0], s[1, 1] < s[0, 1])
                image_ok = torch.logical_and(s[0, 0] < s[0, 1], s[1, 1] < s[1, 0])
                out[f"scores_{mode}"] = torch.stack([s[0, 0], s[0, 1], s[1, 0], s[1, 1]])
                if mode == "text":
                    results_cond["text"] = text_ok
                elif mode == "image":
                    results_cond["image"] = image_ok
                elif cfg_get(ev, "wino_group_conditional", False):
                    results_cond["group"] = torch.logical_and(results_cond["text"], results_cond["image"])
                else:
                    results_cond["group"] = torch.logical_and(image_ok, text_ok)
            bsz = a[0, 0].shape[0]
            for mode, name in (("text", "win_text_accuracy"), ("image", "win_image_accuracy"), ("group", "win_group_accuracy")):
                out[f"{mode}_correct"] = results_cond[mode]
                out[name] = results_cond[mode].sum().item() / bsz
                self._zero_shot_update(name, out[name])
            return out
        x0 = batch["input_ids"]
        sim = self.get_similarity_ar if ar else self.get_similarity
        if cfg_get(ev, "only_one_correct", False):
            # rows 1.. get the image of the NEXT row (rolled within rows 1..): only row 0 keeps its own pair (:577-591)
            x0c = x0.clone()
            second_half = x0c[1:, Lt:]
            x0c[1:, Lt:] = torch.cat([second_half[1:], second_half[0].unsqueeze(0)], dim=0)
            class_sim = sim(x0c, batch, do_unconditional=True)
            acc = (class_sim.topk(k=1, dim=0, largest=False).indices == 0).float().mean().item()
            self._zero_shot_update("datacomp_img_acc", acc)
            return dict(class_sim=class_sim, datacomp_img_acc=acc)
        x0_txt, x0_img = x0.clone(), x0.clone()
        x0_txt[:, :Lt] = x0[0, :Lt]      # image retrieval given text: every row gets the first text (:630)
        x0_img[:, Lt:] = x0[0, Lt:]      # text retrieval given image: every row gets the first image (:633)
        txt_class_sim = sim(x0_txt, batch, txt_cond=True)
        img_class_sim = sim(x0_img, batch, txt_cond=True if ar else False)
        img_acc = (img_class_sim.topk(k=1, dim=0, largest=False).indices == 0).float().mean().item()
        txt_acc = (txt_class_sim.topk(k=1, dim=0, largest=False).indices == 0).float().mean().item()
        self._zero_shot_update("datacomp_img_acc", img_acc)
        self._zero_shot_update("datacomp_txt_acc", txt_acc)
        return dict(txt_class_sim=txt_class_sim, img_class_sim=img_class_sim, datacomp_img_acc=img_acc, datacomp_txt_acc=txt_acc)
