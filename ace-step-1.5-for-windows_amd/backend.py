"""The reference's backend seam, re-implemented for the native MI355X path.

The reference selects an alternate DiT / VAE backend through handler flags and a pair of mixin methods introduced
for MLX:
  * ``_init_mlx_dit`` / ``_init_mlx_vae``   (handler/mlx_dit_init.py:9-43, handler/mlx_vae_init.py:12-96)
  * ``_mlx_run_diffusion``                  (handler/diffusion.py:18-140), called from
    ``_execute_service_generate_diffusion`` (handler/service_generate_execute.py:144-194)
  * ``_mlx_vae_decode`` via ``tiled_decode`` (handler/vae_decode.py:39-48, handler/generate_music_decode.py:165-167)

``NativeDitMixin`` / ``NativeVaeMixin`` provide the same-shaped methods over the C ABI, so a maintainer mixes them
into ``AceStepHandler``.  Because the reference's Python cannot travel to the GPU box,
``NativeHandler`` is this repo's own counterpart of the handler for that path: ``initialize_service`` /
``service_generate`` / ``generate_music`` with the reference's keyword names and return-dict shapes, fed by
pre-embedded conditioning tensors instead of raw text (the text/LM stages are out of scope).

Error contract (reference): backend failure = Python exception, caught at the seam, fall back / error payload;
``generate_music`` never raises (handler/generate_music.py:181-190).  The native methods themselves never fall back
to a CPU implementation: a missing library or a failed HIP call raises ``RuntimeError``.
"""
from __future__ import annotations

import contextlib
import inspect
import logging
import os
import time
import traceback
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from .config import DitConfig, TextEncoderConfig, VaeConfig

logger = logging.getLogger("ace355")

MAX_BATCH_SIZE = 8  # handler/service_generate_request.py:12
_ALIGN_POST_ENV = os.environ.get("ACE355_ALIGN_POST", "") == "1"   # read once: the default of NativeDitMixin.native_lyric_post
_LM_SAMPLER_ENV = os.environ.get("ACE355_LM_SAMPLER", "") == "1"   # read once: the default of NativeLmMixin.use_native_lm_sampler
_LM_LOOP_ENV = os.environ.get("ACE355_LM_LOOP", "") == "1"         # read once: the default of NativeLmMixin.use_native_lm_loop
_LM_BATCH_ENV = os.environ.get("ACE355_LM_BATCH", "") == "1"       # read once: the default of NativeLmMixin.use_native_lm_batch
_LM_NOCFG_ENV = os.environ.get("ACE355_LM_NOCFG", "") == "1"       # read once: the default of NativeLmMixin.use_native_lm_nocfg
_LM_SCORE_ENV = os.environ.get("ACE355_LM_SCORE", "") == "1"       # read once: the default of NativeLmMixin.use_native_lm_score
_LM_GQA4_ENV = os.environ.get("ACE355_LM_GQA4", "") == "1"         # read once: the default of NativeLmMixin.use_native_lm_gqa4
_AUDIO_IN_ENV = os.environ.get("ACE355_AUDIO_IN", "") == "1"       # read once: the default of NativeAudioInMixin.use_native_audio_in
_FLAC_GPU_ENV = os.environ.get("ACE355_FLAC_GPU", "") == "1"       # read once: the default of NativeAudioInMixin.native_flac_decode


class NativeDitMixin:
    """Required host attributes: ``model`` (with ``.decoder``, ``.null_condition_emb``, ``.config``), ``device``, ``dtype``."""

    use_native_dit: bool = False
    native_dit = None
    # opt-in: get_lyric_timestamp / get_lyric_score run the stage after the maps on the GPU too (ace355.align_post) instead of handing a
    # [layers, 16, L, S] stack to the host's aligners; ACE355_ALIGN_POST=1 turns it on for every host
    native_lyric_post: bool = _ALIGN_POST_ENV

    def _init_native_dit(self) -> bool:
        """Counterpart of ``_init_mlx_dit``: convert weights from the already-loaded PyTorch module. Never raises."""
        try:
            quant = getattr(self, "quantization", None)
            # the reference's quantization knob (init_service_loader.py:89-113): "fp8_weight_only" has a native counterpart (same
            # numerics: per-channel e4m3 weights, bf16 arithmetic); the int8 schemes do not
            if getattr(self, "use_lora", False) or (quant and quant != "fp8_weight_only") or getattr(self, "offload_to_cpu", False):
                logger.info("[native-dit] LoRA / int8 quantization / CPU offload active; keeping the PyTorch path")
                self.use_native_dit, self.native_dit = False, None
                return False
            from .dit import NativeDit
            cfg = DitConfig.from_reference(self.model.config) if not isinstance(getattr(self.model, "config", None), DitConfig) \
                else self.model.config
            dit = NativeDit(cfg, self.device)
            dit.load_state_dict(self.model.decoder.state_dict())
            if quant == "fp8_weight_only":
                dit.set_precision("fp8_weight_only")
            self.native_dit, self.use_native_dit = dit, True
            self._native_adapter_key = None   # (a fresh handle carries the base weights)
            logger.info("[native-dit] decoder packed for gfx950 (%d layers, hidden %d)", cfg.num_hidden_layers, cfg.hidden_size)
            return True
        except Exception as exc:  # same policy as handler/mlx_dit_init.py:36-43
            logger.warning("[native-dit] init failed (%s: %s); PyTorch path stays active", type(exc).__name__, exc)
            self.use_native_dit, self.native_dit = False, None
            return False

    def _native_adapter_terms(self):
        """The LoRA / LoKr terms the native DiT should carry now.  Default: the PEFT-wrapped ``self.model.decoder`` and its LyCORIS
        network (the reference loads adapters there after ``initialize_service``, H/lora/lifecycle.py:164-283), read by duck typing.  Hosts with a registry of their
        own override this (``NativeHandler``)."""
        from .lora import terms_from_decoder
        return terms_from_decoder(self.model.decoder, getattr(self.native_dit, "cfg", None), allow_dora=True)

    def _sync_native_adapters(self) -> None:
        """Bring the native DiT's merged adapters in line with the host's: nothing at all while ``use_lora`` is off and nothing is
        applied; a re-merge when the terms' fingerprint (names, scales, tensors, in-place versions) changed; the base back when
        ``use_lora`` turned off.  ``UnsupportedAdapter`` (Tucker LoKr, trained biases, ...) propagates."""
        applied = getattr(self, "_native_adapter_key", None)
        if not getattr(self, "use_lora", False):
            if applied is not None:
                self.native_dit.clear_adapters()
                self._native_adapter_key = None
            return
        from .lora import fingerprint
        terms = list(self._native_adapter_terms())
        key = fingerprint(terms) if terms else None
        if key == applied:
            return
        if terms:
            self.native_dit.set_adapters(terms)
        else:
            self.native_dit.clear_adapters()
        self._native_adapter_key = key

    def _model_honours_timesteps(self) -> bool:
        """Whether the loaded checkpoint's own ``generate_audio`` reads an explicit ``timesteps=``: the sft and turbo models do
        (sft/modeling_acestep_v15_base.py:1864-1875, turbo :1807-1865); the BASE model has no such parameter - it lands in
        ``**kwargs`` and the schedule is always linspace + shift (base/modeling_acestep_v15_base.py:1812, 1864-1867).  The
        native path must not diverge from the checkpoint it stands in for.  ``model_variant`` ("base" | "sft" | "turbo") on
        the host overrides the signature probe (``NativeHandler`` has no reference module to probe)."""
        variant = getattr(self, "model_variant", None)
        if variant is not None:
            return variant in ("sft", "turbo")
        ga = getattr(getattr(self, "model", None), "generate_audio", None)
        if ga is None:
            return True
        try:
            return "timesteps" in inspect.signature(ga).parameters
        except (TypeError, ValueError):
            return True

    def _is_turbo(self) -> bool:
        """handler/init_service_catalog.py:69-73 (`is_turbo_model`): a ``config.is_turbo`` flag on the host, or
        ``model_variant == "turbo"``."""
        return bool(getattr(getattr(self, "config", None), "is_turbo", False)) or getattr(self, "model_variant", None) == "turbo"

    def _native_run_diffusion(
        self,
        encoder_hidden_states,
        encoder_attention_mask,
        context_latents,
        src_latents,
        seed,
        infer_method: str = "ode",
        shift: float = 3.0,
        timesteps=None,
        audio_cover_strength: float = 1.0,
        encoder_hidden_states_non_cover=None,
        encoder_attention_mask_non_cover=None,
        context_latents_non_cover=None,
        disable_tqdm: bool = False,
        # base/sft knobs the MLX path lacks (handler/service_generate_execute.py:78-104)
        infer_steps: int = 30,
        guidance_scale: float = 7.0,
        cfg_interval_start: float = 0.0,
        cfg_interval_end: float = 1.0,
        use_adg: bool = False,
        cover_noise_strength: float = 0.0,
    ) -> Dict[str, Any]:
        """Same contract as ``_mlx_run_diffusion`` (handler/diffusion.py:18-140): returns
        ``{"target_latents": Tensor[B,T,64] on self.device in self.dtype, "time_costs": {...}}``.
        The attention masks are accepted and unused: the DiT discards them (modeling_acestep_v15_base.py:1384-1385)."""
        _ = encoder_attention_mask, encoder_attention_mask_non_cover, disable_tqdm
        for attr in ("native_dit", "device", "dtype", "model"):
            if not hasattr(self, attr):
                raise AttributeError(f"NativeDitMixin host is missing required attribute '{attr}'")
        if self.native_dit is None:
            raise RuntimeError("native DiT backend is not initialised (call _init_native_dit)")
        if infer_method not in {"ode", "sde"}:
            raise ValueError(f"Unsupported infer_method '{infer_method}'. Expected 'ode' or 'sde'.")
        if timesteps is not None and not (hasattr(timesteps, "__iter__") or hasattr(timesteps, "tolist")):
            raise TypeError("timesteps must be iterable, tensor-like, or None")
        if encoder_hidden_states.shape[0] != context_latents.shape[0]:
            raise ValueError("Batch dimension mismatch: encoder_hidden_states and context_latents must share dim 0")
        if encoder_hidden_states.shape[0] != src_latents.shape[0]:
            raise ValueError("Batch dimension mismatch: encoder_hidden_states and src_latents must share dim 0")
        if encoder_hidden_states_non_cover is not None and encoder_hidden_states_non_cover.shape[0] != encoder_hidden_states.shape[0]:
            raise ValueError("Batch dimension mismatch: encoder_hidden_states_non_cover must share dim 0 with encoder_hidden_states")
        if context_latents_non_cover is not None and context_latents_non_cover.shape[0] != context_latents.shape[0]:
            raise ValueError("Batch dimension mismatch: context_latents_non_cover must share dim 0 with context_latents")
        ts_list = None
        if timesteps is not None:
            ts_list = timesteps.tolist() if hasattr(timesteps, "tolist") else list(timesteps)
        if ts_list is not None and not self._is_turbo() and not self._model_honours_timesteps():
            logger.info("[native-dit] base checkpoint: explicit timesteps are ignored, as its generate_audio does")
            ts_list = None
        self._sync_native_adapters()   # (UnsupportedAdapter propagates: the seam's except runs the PyTorch path)
        if self._is_turbo():
            # turbo checkpoints (handler init_service_catalog.py:69-73 `is_turbo_model`): the model's own generate_audio has no
            # CFG / step count, only the shift -> 8-step table (turbo modeling file :1780-1995); same native loop
            from .dit import generate_latents_turbo
            out = generate_latents_turbo(
                self.native_dit, encoder_hidden_states, context_latents, seed=seed, shift=shift, timesteps=ts_list,
                infer_method=infer_method, audio_cover_strength=audio_cover_strength, cover_noise_strength=cover_noise_strength,
                src_latents=src_latents, encoder_hidden_states_non_cover=encoder_hidden_states_non_cover,
                context_latents_non_cover=context_latents_non_cover)
            out["target_latents"] = out["target_latents"].to(device=self.device, dtype=self.dtype)
            return out
        from .dit import generate_latents
        out = generate_latents(
            self.native_dit, self.model.null_condition_emb.detach(), encoder_hidden_states, context_latents, seed=seed,
            infer_method=infer_method, infer_steps=infer_steps, diffusion_guidance_sale=guidance_scale,
            cfg_interval_start=cfg_interval_start, cfg_interval_end=cfg_interval_end, use_adg=use_adg, shift=shift,
            timesteps=ts_list, audio_cover_strength=audio_cover_strength, cover_noise_strength=cover_noise_strength,
            src_latents=src_latents, encoder_hidden_states_non_cover=encoder_hidden_states_non_cover,
            context_latents_non_cover=context_latents_non_cover)
        out["target_latents"] = out["target_latents"].to(device=self.device, dtype=self.dtype)
        return out

    # ---------------------------------------------------------------- lyric alignment (H/lyric_timestamp.py, H/lyric_score.py)
    def _lyric_layers_config(self, custom_layers_config=None):
        """The caller's config, else the host's ``custom_layers_config`` (acestep/handler.py:129), else the reference default."""
        if custom_layers_config is not None:
            return custom_layers_config
        from .align import DEFAULT_LAYERS_HEADS
        return getattr(self, "custom_layers_config", None) or DEFAULT_LAYERS_HEADS

    def lyric_attention(self, pred_latent, encoder_hidden_states, context_latents, inference_steps: int = 8, seed: Optional[int] = 42,
                        custom_layers_config=None, kind: str = "timestamp"):
        """The cross-attention maps of the reference's alignment forward on the native DiT, in the handlers' layout and the host's dtype
        (``ace355.align.lyric_attention``): one stack for ``kind="timestamp"``, an (lm, dit) pair for ``"score"``."""
        if self.native_dit is None:
            raise RuntimeError("native DiT backend is not initialised (call _init_native_dit)")
        self._sync_native_adapters()
        from .align import lyric_attention
        return lyric_attention(self.native_dit, pred_latent, encoder_hidden_states, context_latents, inference_steps, seed,
                               self._lyric_layers_config(custom_layers_config), kind, getattr(self, "dtype", torch.bfloat16))

    def _lyric_segment(self, lyric_token_ids, vocal_language: str):
        """The lyric token range: after the "# Languages / # Lyric" header the text encoder saw, up to <|endoftext|> (151643)."""
        ids = lyric_token_ids[0].tolist() if isinstance(lyric_token_ids, torch.Tensor) else list(lyric_token_ids)
        tok = getattr(self, "text_tokenizer", None)
        if tok is None:
            raise RuntimeError("lyric alignment needs the host's text_tokenizer")
        start = len(tok.encode(f"# Languages\n{vocal_language}\n\n# Lyric\n", add_special_tokens=False))
        end = ids.index(151643) if 151643 in ids else len(ids)
        return ids[start:end], start, end

    def _lyric_maps(self, pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers, kind):
        """The fp32 maps [n_pairs, N, L, S] of the alignment forward, where the native DiT wrote them (``ace355.align.lyric_maps``)."""
        self._sync_native_adapters()
        from .align import lyric_maps
        maps, _prs, bsz = lyric_maps(self.native_dit, pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers,
                                     kind, getattr(self, "dtype", torch.bfloat16))
        if bsz != 1:
            raise ValueError("the native lyric stage takes one item per call, as the aligners do")
        return maps

    def _native_lyric_timestamp(self, pred_latent, encoder_hidden_states, context_latents, lyric_token_ids, total_duration_seconds,
                                vocal_language, inference_steps, seed, layers) -> Optional[Dict[str, Any]]:
        """``get_lyric_timestamp`` with the whole stage native (``native_lyric_post``): maps -> consensus matrix -> DTW on the GPU, one
        synchronisation for the token spans, text on the host.  None when anything raises: the caller goes on with the host aligners."""
        try:
            from . import align_post
            maps = self._lyric_maps(pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers, "timestamp")
            ids, start, end = self._lyric_segment(lyric_token_ids, vocal_language)
            res = align_post.lyric_timestamps(maps, 0, start, end, self.text_tokenizer, ids, total_duration_seconds,
                                              dtype=getattr(self, "dtype", torch.bfloat16), violence_level=2.0, medfilt_width=1)
            return {"lrc_text": res["lrc_text"], "sentence_timestamps": res["sentence_timestamps"],
                    "token_timestamps": res["token_timestamps"], "success": True, "error": None}
        except Exception as exc:
            logger.warning("[get_lyric_timestamp] native alignment stage failed (%s: %s); using the host aligner", type(exc).__name__, exc)
            return None

    def _native_lyric_score(self, pred_latent, encoder_hidden_states, context_latents, lyric_token_ids, vocal_language, inference_steps,
                            seed, layers) -> Optional[Dict[str, Any]]:
        """``get_lyric_score`` with the whole stage native: the lm and dit matrices go through the DTW and the metrics as one batch."""
        try:
            from . import align_post
            maps = self._lyric_maps(pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers, "score")
            ids, start, end = self._lyric_segment(lyric_token_ids, vocal_language)
            if start >= maps.shape[-2]:
                return self._score_error("Lyrics indices out of bounds")
            lm, dit = align_post.lyric_scores(maps, (0, 1), start, end, self.text_tokenizer, ids,
                                              dtype=getattr(self, "dtype", torch.bfloat16), medfilt_width=1)
            return {"lm_score": lm, "dit_score": dit, "success": True, "error": None}
        except Exception as exc:
            logger.warning("[get_lyric_score] native alignment stage failed (%s: %s); using the host aligner", type(exc).__name__, exc)
            return None

    @staticmethod
    def _timestamp_error(message: str) -> Dict[str, Any]:
        return {"lrc_text": "", "sentence_timestamps": [], "token_timestamps": [], "success": False, "error": message}

    @staticmethod
    def _score_error(message: str) -> Dict[str, Any]:
        return {"lm_score": 0.0, "dit_score": 0.0, "success": False, "error": message}

    # host-side failures of the aligner stage that become an error payload (the reference's list, plus a missing scoring package or tokenizer)
    _ALIGN_ERRORS = (ValueError, KeyError, RuntimeError, OSError, ImportError, AttributeError)

    @torch.inference_mode()
    def get_lyric_timestamp(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents, lyric_token_ids,
                            total_duration_seconds: float, vocal_language: str = "en", inference_steps: int = 8, seed: int = 42,
                            custom_layers_config=None) -> Dict[str, Any]:
        """``get_lyric_timestamp`` (H/lyric_timestamp.py) with the maps from the native DiT; the host's ``MusicStampsAligner`` turns them into
        LRC.  Without an active native DiT, or when the native part raises, the host's own method (further up the MRO) runs; a host without
        one gets the error payload.  ``encoder_attention_mask`` is accepted and unused: the DiT discards it (base.py:1384-1385)."""
        args = dict(pred_latent=pred_latent, encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                    context_latents=context_latents, lyric_token_ids=lyric_token_ids, total_duration_seconds=total_duration_seconds,
                    vocal_language=vocal_language, inference_steps=inference_steps, seed=seed, custom_layers_config=custom_layers_config)
        parent = getattr(super(), "get_lyric_timestamp", None)
        if not (self.use_native_dit and self.native_dit is not None):
            return parent(**args) if parent else self._timestamp_error("no lyric alignment backend available: the native DiT is not active")
        if not isinstance(inference_steps, int) or inference_steps <= 0:
            return self._timestamp_error(f"inference_steps must be a positive non-zero integer, got {inference_steps!r}")
        layers = self._lyric_layers_config(custom_layers_config)
        if self.native_lyric_post:
            res = self._native_lyric_timestamp(pred_latent, encoder_hidden_states, context_latents, lyric_token_ids, total_duration_seconds,
                                               vocal_language, inference_steps, seed, layers)
            if res is not None:
                return res
        try:
            matrix = self.lyric_attention(pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers, "timestamp")
        except Exception as exc:
            logger.warning("[get_lyric_timestamp] native cross-attention maps failed (%s: %s)", type(exc).__name__, exc)
            if parent:
                return parent(**args)
            return self._timestamp_error(f"Error generating timestamps: {exc}")
        try:
            ids, start, end = self._lyric_segment(lyric_token_ids, vocal_language)
            from acestep.core.scoring.dit_alignment import MusicStampsAligner
            aligner = MusicStampsAligner(self.text_tokenizer)
            info = aligner.stamps_align_info(attention_matrix=matrix[:, :, start:end, :], lyrics_tokens=ids,
                                             total_duration_seconds=total_duration_seconds, custom_config=layers, return_matrices=False,
                                             violence_level=2.0, medfilt_width=1)
            if info.get("calc_matrix") is None:
                return self._timestamp_error(info.get("error", "Failed to process attention matrix"))
            res = aligner.get_timestamps_and_lrc(calc_matrix=info["calc_matrix"], lyrics_tokens=ids,
                                                 total_duration_seconds=total_duration_seconds)
            return {"lrc_text": res["lrc_text"], "sentence_timestamps": res["sentence_timestamps"],
                    "token_timestamps": res["token_timestamps"], "success": True, "error": None}
        except self._ALIGN_ERRORS as exc:
            logger.warning("[get_lyric_timestamp] failed (%s: %s)", type(exc).__name__, exc)
            return self._timestamp_error(f"Error generating timestamps: {exc}")

    @torch.inference_mode()
    def get_lyric_score(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents, lyric_token_ids,
                        vocal_language: str = "en", inference_steps: int = 8, seed: int = 42, custom_layers_config=None) -> Dict[str, Any]:
        """``get_lyric_score`` (H/lyric_score.py) with the maps of its noise rows (lm) and mixed rows (dit) from the native DiT; the host's
        ``MusicLyricScorer`` scores them.  Fallback and error payloads as ``get_lyric_timestamp``."""
        args = dict(pred_latent=pred_latent, encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                    context_latents=context_latents, lyric_token_ids=lyric_token_ids, vocal_language=vocal_language,
                    inference_steps=inference_steps, seed=seed, custom_layers_config=custom_layers_config)
        parent = getattr(super(), "get_lyric_score", None)
        if not (self.use_native_dit and self.native_dit is not None):
            return parent(**args) if parent else self._score_error("no lyric alignment backend available: the native DiT is not active")
        if not isinstance(inference_steps, int) or inference_steps <= 0:
            return self._score_error(f"Error generating score: inference_steps must be a positive non-zero integer, got {inference_steps!r}")
        layers = self._lyric_layers_config(custom_layers_config)
        if self.native_lyric_post:
            res = self._native_lyric_score(pred_latent, encoder_hidden_states, context_latents, lyric_token_ids, vocal_language,
                                           inference_steps, seed, layers)
            if res is not None:
                return res
        try:
            lm, dit = self.lyric_attention(pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers, "score")
        except Exception as exc:
            logger.warning("[get_lyric_score] native cross-attention maps failed (%s: %s)", type(exc).__name__, exc)
            if parent:
                return parent(**args)
            return self._score_error(f"Error generating score: {exc}")
        try:
            ids, start, end = self._lyric_segment(lyric_token_ids, vocal_language)
            if start >= lm.shape[-2]:
                return self._score_error("Lyrics indices out of bounds")
            from acestep.core.scoring.dit_score import MusicLyricScorer
            aligner = MusicLyricScorer(self.text_tokenizer)

            def one(matrix):
                info = aligner.lyrics_alignment_info(attention_matrix=matrix[..., start:end, :], token_ids=ids, custom_config=layers,
                                                     return_matrices=False, medfilt_width=1)
                if info.get("energy_matrix") is None:
                    return 0.0
                res = aligner.calculate_score(energy_matrix=info["energy_matrix"], type_mask=info["type_mask"],
                                              path_coords=info["path_coords"])
                return float(res.get("lyrics_score", res.get("final_score", 0.0)))
            return {"lm_score": one(lm), "dit_score": one(dit), "success": True, "error": None}
        except self._ALIGN_ERRORS as exc:
            logger.warning("[get_lyric_score] failed (%s: %s)", type(exc).__name__, exc)
            return self._score_error(f"Error generating score: {exc}")


class NativeVaeMixin:
    """Required host attributes: ``vae`` (state_dict + config) or ``vae_state_dict``/``vae_config``, ``device``."""

    use_native_vae: bool = False
    native_vae = None

    def _init_native_vae(self) -> bool:
        """Counterpart of ``_init_mlx_vae``: fuse weight-norm + pack from the loaded ``AutoencoderOobleck``. Never raises."""
        try:
            from .vae import NativeVae
            vae_mod = getattr(self, "vae", None)
            cfg = getattr(self, "vae_config", None)
            if cfg is None:
                cfg = VaeConfig.from_reference(vae_mod.config)
            sd = getattr(self, "vae_state_dict", None) or vae_mod.state_dict()
            nv = NativeVae(cfg, self.device)
            nv.load_state_dict(sd)
            self.native_vae, self.use_native_vae = nv, True
            logger.info("[native-vae] decoder packed for gfx950 (hop %d)", nv.hop)
            return True
        except Exception as exc:
            logger.warning("[native-vae] init failed (%s: %s); PyTorch path stays active", type(exc).__name__, exc)
            self.use_native_vae, self.native_vae = False, None
            return False

    def _native_vae_decode(self, latents: torch.Tensor) -> torch.Tensor:
        """``latents [B,64,T]`` -> fp32 waveform ``[B,2,hop*T]`` on the device (``_mlx_vae_decode`` returns CPU fp32;
        both are accepted downstream: ``.float()``, ``amax``, ``.cpu()`` follow, handler/generate_music_decode.py:191)."""
        if self.native_vae is None:
            raise RuntimeError("native VAE backend is not initialised (call _init_native_vae)")
        return self.native_vae.decode(latents)

    def _native_vae_encode_sample(self, audio: torch.Tensor) -> torch.Tensor:
        """``audio [B,2,L]`` -> sampled latents fp32 ``[B,64,T]`` (counterpart of ``_mlx_vae_encode_sample``,
        handler/vae_encode.py:33: whole-sequence encode; the 30 s / 2 s-overlap tiling is a memory workaround)."""
        if self.native_vae is None or not getattr(self.native_vae, "has_encoder", False):
            raise RuntimeError("native VAE encoder is not initialised (encoder.* weights missing)")
        return self.native_vae.encode(audio)

    def tiled_encode(self, audio, chunk_size=None, overlap=None, offload_latent_to_cpu=True):
        """Same signature as handler/vae_encode.py:15-86.  Native fast path first; on failure the host's PyTorch
        implementation (``VaeEncodeMixin.tiled_encode`` further up the MRO) runs, exactly like the MLX seam (:28-45)."""
        if self.use_native_vae and self.native_vae is not None and getattr(self.native_vae, "has_encoder", False):
            input_was_2d = audio.dim() == 2
            try:
                result = self._native_vae_encode_sample(audio.unsqueeze(0) if input_was_2d else audio)
                return result.squeeze(0) if input_was_2d else result
            except Exception as exc:
                logger.warning("[tiled_encode] native VAE encode failed (%s: %s)", type(exc).__name__, exc)
        parent = getattr(super(), "tiled_encode", None)
        if parent is None:
            raise RuntimeError("no VAE encode backend available")
        return parent(audio, chunk_size=chunk_size, overlap=overlap, offload_latent_to_cpu=offload_latent_to_cpu)

    def tiled_decode(self, latents, chunk_size: Optional[int] = None, overlap: int = 64, offload_wav_to_cpu: Optional[bool] = None):
        """Same signature as handler/vae_decode.py:16-85.  Native fast path first (whole-sequence decode, which equals
        the overlap-discard tiling up to fp summation order); on failure the host's PyTorch
        ``_tiled_decode_inner`` runs if the host has one, exactly like the MLX seam (handler/vae_decode.py:39-48)."""
        if self.use_native_vae and self.native_vae is not None:
            try:
                return self._native_vae_decode(latents)
            except Exception as exc:
                logger.warning("[tiled_decode] native VAE decode failed (%s: %s)", type(exc).__name__, exc)
                if not hasattr(self, "_tiled_decode_inner"):
                    raise
        if not hasattr(self, "_tiled_decode_inner"):
            raise RuntimeError("no VAE decode backend available")
        if chunk_size is None:
            chunk_size = self._get_auto_decode_chunk_size()
        if offload_wav_to_cpu is None:
            offload_wav_to_cpu = self._should_offload_wav_to_cpu()
        return self._tiled_decode_inner(latents, chunk_size, overlap, offload_wav_to_cpu)


class NativeTextEncoderMixin:
    """Required host attributes: ``text_encoder`` (the loaded ``Qwen3Model``), ``device``; optional ``offload_to_cpu``."""

    use_native_text_encoder: bool = False

    def _init_native_text_encoder(self) -> bool:
        """Swap ``self.text_encoder`` for ``modswap.NativeTextEncoderSwap`` (the PyTorch module stays inside as the per-call fallback;
        its state_dict keys are unchanged).  Same policy as ``_init_native_dit``: refused under CPU offload or off a CUDA device, and any
        failure is logged and leaves the PyTorch module in place.  Never raises."""
        try:
            if getattr(self, "offload_to_cpu", False) or not str(getattr(self, "device", "cpu")).startswith("cuda"):
                logger.info("[native-text-encoder] CPU offload active or no GPU device; keeping the PyTorch path")
                self.use_native_text_encoder = False
                return False
            if getattr(self, "text_encoder", None) is None:
                raise RuntimeError("no text encoder loaded")
            from .modswap import native_of, swap_in_text_encoder
            wrapper = swap_in_text_encoder(self, self.device)
            self.use_native_text_encoder = True
            cfg = native_of(wrapper).cfg
            logger.info("[native-text-encoder] packed for gfx950 (%d layers, hidden %d)", cfg.num_hidden_layers, cfg.hidden_size)
            return True
        except Exception as exc:
            logger.warning("[native-text-encoder] init failed (%s: %s); PyTorch path stays active", type(exc).__name__, exc)
            self.use_native_text_encoder = False
            return False


class NativeLmMixin:
    """For the reference's ``LLMHandler``.  Required host attributes: ``llm`` (the loaded ``Qwen3ForCausalLM``), ``device``; optional
    ``offload_to_cpu``, ``native_lm_max_positions`` (cache positions: prompt + generated tokens, default 8192)."""

    use_native_lm: bool = False
    # Four q heads per kv head (``acestep-5Hz-lm-4B``: Qwen3-4B, 32 / 8 heads) are served only to a host that asks: with this flag
    # set (ACE355_LM_GQA4=1 turns it on for every host) the swap below passes ``allow_gqa4=True`` down to ``ace355_lm_create_ex``.
    # Without it a 4B host logs the refusal and keeps PyTorch, as before.  Opt-in because the layout is unpinned on trained weights
    # and its native copy costs 8 GB beside the module.
    use_native_lm_gqa4: bool = _LM_GQA4_ENV

    def _init_native_lm(self) -> bool:
        """Swap ``self.llm`` for ``modswap.NativeCausalLMSwap`` after the model is loaded: ``_forward_pass``'s prefill and decode steps
        then run natively, and everything else (``generate``, the sampling code around the logits) is untouched.  Same policy as
        ``_init_native_text_encoder``: refused under CPU offload or off a CUDA device, any failure is logged and leaves the PyTorch
        module in place.  Never raises."""
        try:
            if getattr(self, "offload_to_cpu", False) or not str(getattr(self, "device", "cpu")).startswith("cuda"):
                logger.info("[native-lm] CPU offload active or no GPU device; keeping the PyTorch path")
                self.use_native_lm = False
                return False
            if getattr(self, "llm", None) is None:
                raise RuntimeError("no LM loaded")
            from . import modswap
            opt_in = {"allow_gqa4": True} if self.use_native_lm_gqa4 else {}
            wrapper = modswap.swap_in_lm(self, self.device, max_positions=int(getattr(self, "native_lm_max_positions", 8192)), **opt_in)
            self.use_native_lm = True
            cfg = modswap.native_of(wrapper).cfg
            logger.info("[native-lm] packed for gfx950 (%d layers, hidden %d, %d / %d heads, vocabulary %d)", cfg.num_hidden_layers,
                        cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.vocab_size)
            return True
        except Exception as exc:
            logger.warning("[native-lm] init failed (%s: %s); PyTorch path stays active", type(exc).__name__, exc)
            self.use_native_lm = False
            return False

    # ------------------------------------------------------------------ the quality score (opt-in)
    # ``ace355.lmscore`` carries the reference's scoring entry points (acestep/core/scoring/lm_score.py) on ``NativeCausalLM.score``:
    # per target token one log-probability and one rank from the GPU instead of [T, V] logits on the host.  It takes the native path
    # only with this flag set (ACE355_LM_SCORE=1 turns it on for every host); ranks among EQUAL logits are by ascending id there,
    # where torch.topk's order is unspecified, which is why it is opt-in.
    use_native_lm_score: bool = _LM_SCORE_ENV

    def get_hf_model_for_scoring(self):
        """The reference's scoring reads the logits of EVERY position of ``model(input_ids, attention_mask)``; the native swap answers
        that call with the last column only ([1, 1, V]).  On the ``pt`` backend with the swap installed this therefore hands out the
        kept ``Qwen3ForCausalLM`` instead of ``self.llm``; everything else is the host's own answer."""
        from . import modswap
        llm = getattr(self, "llm", None)
        if getattr(self, "llm_backend", "pt") == "pt" and isinstance(llm, modswap.NativeCausalLMSwap):
            return llm._reference
        return super().get_hf_model_for_scoring()

    # ------------------------------------------------------------------ token selection (opt-in)
    # The reference's loops call _apply_top_k_filter, _apply_top_p_filter and _sample_tokens in that order on one tensor
    # (llm_inference.py:2380-2384, :2496-2500, :3646-3650).  With ``use_native_lm_sampler`` the two filters only note what they were asked
    # for and ``_sample_tokens`` does all three in one native call (ace355.lmsample): same distribution, a different draw per seed, which
    # is why it is opt-in; ACE355_LM_SAMPLER=1 turns it on for every host.  Off, or for a tensor that is not on the GPU, nothing changes.
    use_native_lm_sampler: bool = _LM_SAMPLER_ENV
    _lm_sampler_record = None      # [tensor, k, p]: filters deferred for exactly this tensor object
    _lm_sampler_failures = 0

    def _lm_sampler_takes(self, logits) -> bool:
        return bool(self.use_native_lm_sampler) and isinstance(logits, torch.Tensor) and logits.is_cuda

    def _lm_sampler_note(self, logits):
        rec = self._lm_sampler_record
        if rec is None or rec[0] is not logits:   # a record for a different tensor is dropped, never applied
            rec = self._lm_sampler_record = [logits, None, None]
        return rec

    def _apply_top_k_filter(self, logits, top_k):
        if not self._lm_sampler_takes(logits):
            return super()._apply_top_k_filter(logits, top_k)
        self._lm_sampler_record = None   # top-k opens a step: whatever was noted before belongs to another one
        self._lm_sampler_note(logits)[1] = top_k
        return logits

    def _apply_top_p_filter(self, logits, top_p):
        if not self._lm_sampler_takes(logits):
            return super()._apply_top_p_filter(logits, top_p)
        self._lm_sampler_note(logits)[2] = top_p
        return logits

    def _sample_tokens(self, logits, temperature):
        rec, self._lm_sampler_record = self._lm_sampler_record, None
        if not self._lm_sampler_takes(logits):
            return super()._sample_tokens(logits, temperature)
        top_k, top_p = (rec[1], rec[2]) if rec is not None and rec[0] is logits else (None, None)   # else: the caller filtered elsewhere
        try:
            from .lmsample import select_tokens
            return select_tokens(logits, top_k, top_p, temperature)
        except Exception as exc:
            if self._lm_sampler_failures < 3:
                logger.warning("[native-lm-sampler] %s: %s; this step runs on the PyTorch path", type(exc).__name__, exc)
            self._lm_sampler_failures += 1
            logits = super()._apply_top_k_filter(logits, top_k)   # the deferred filters first
            logits = super()._apply_top_p_filter(logits, top_p)
            return super()._sample_tokens(logits, temperature)

    # ------------------------------------------------------------------ the CFG loop (opt-in)
    # With ``use_native_lm_loop`` (ACE355_LM_LOOP=1 for every host) ``_generate_with_cfg_custom`` is ace355.lmlogits.generate_with_cfg:
    # the logits stage between forward and selection is one native launch, and a codes-phase token goes forward -> stage -> selection
    # -> next forward without the host reading it.  The flag implies the native selection whatever ``use_native_lm_sampler`` says: the
    # distribution is the reference's, the draw for a given seed is ace355.lmsample's (one torch.rand(B) per step), not
    # torch.multinomial's.  The call goes to the reference's loop, untouched, when the flag is off, ``self.llm`` is not the native
    # swap, the ids are not on a CUDA device, the attention mask is not left-padded, or the request exceeds the native handle
    # (2B > max_seqs, P + max_new_tokens > max_positions, 2B * P > 65536, vocabulary > 1 << 20).  With the flag on, each such reason
    # is logged once per handler (``[native-lm-loop] ...``), so a loop that never runs natively does not go unnoticed.
    use_native_lm_loop: bool = _LM_LOOP_ENV
    _lm_loop_stats = None   # of the last native call: {"steps", "native_steps", "sync_free_steps", "token_reads"}

    _lm_loop_reasons_logged = frozenset()

    def _lm_loop_native(self, batch_input_ids, batch_attention_mask, max_new_tokens):
        """``(the NativeCausalLM the loop would run on, None)``, or ``(None, why)`` when the call belongs to the reference's loop
        (``why`` is None with the flag off: nothing was asked for)."""
        if not self.use_native_lm_loop:
            return None, None
        return self._lm_loop_accepts(batch_input_ids, batch_attention_mask, max_new_tokens)

    def _lm_loop_accepts(self, batch_input_ids, batch_attention_mask, max_new_tokens, pairs=True):
        """``_lm_loop_native`` whatever ``use_native_lm_loop`` says (the batched path below implies the native loop).  ``pairs``
        False: the rows are N = B >= 1 prompts of the non-CFG loop, not conditional + unconditional ones."""
        if not isinstance(batch_input_ids, torch.Tensor) or not batch_input_ids.is_cuda or batch_input_ids.dim() != 2:
            return None, f"the input ids are not a [{'2B' if pairs else 'B'}, P] tensor on a CUDA device"
        from . import lm as _lm, modswap, native
        llm = modswap.native_of(getattr(self, "llm", None))
        if not isinstance(llm, _lm.NativeCausalLM):
            return None, "self.llm is not the native LM (see _init_native_lm)"
        if batch_input_ids.device != llm.device:
            return None, f"the input ids are on {batch_input_ids.device}, the native LM on {llm.device}"
        N, P = batch_input_ids.shape
        if pairs and (N < 2 or N % 2 or P < 1):
            return None, f"{N} x {P} input ids are not conditional + unconditional rows"
        if N < 1 or P < 1:
            return None, f"{N} x {P} input ids hold no prompt"
        if N > llm.max_seqs or P + int(max_new_tokens) > llm.max_positions or N * P > native.LM_MAX_TOKENS:
            return None, (f"{N} sequences of {P} + {int(max_new_tokens)} positions exceed the native handle ({llm.max_seqs} sequences, "
                          f"{llm.max_positions} positions, {native.LM_MAX_TOKENS} prefill tokens)")
        if llm.cfg.vocab_size > native.LM_PICK_MAX_V:
            return None, f"a vocabulary of {llm.cfg.vocab_size} exceeds {native.LM_PICK_MAX_V}"
        if batch_attention_mask is not None:
            if tuple(batch_attention_mask.shape) != (N, P):
                return None, "the attention mask does not have the ids' shape"
            try:
                _lm.left_pad_first(batch_attention_mask)
            except NotImplementedError as exc:
                return None, str(exc)
        return llm, None

    def _generate_with_cfg_custom(self, batch_input_ids, batch_attention_mask, max_new_tokens, temperature, cfg_scale, top_k, top_p,
                                  repetition_penalty, pad_token_id, streamer, constrained_processor=None):
        llm, why = self._lm_loop_native(batch_input_ids, batch_attention_mask, max_new_tokens)
        if llm is None:
            if why is not None and why not in self._lm_loop_reasons_logged:   # once per reason and handler
                self._lm_loop_reasons_logged = self._lm_loop_reasons_logged | {why}
                logger.info("[native-lm-loop] %s; this request runs the reference's loop", why)
            return super()._generate_with_cfg_custom(batch_input_ids, batch_attention_mask, max_new_tokens, temperature, cfg_scale, top_k,
                                                     top_p, repetition_penalty, pad_token_id, streamer, constrained_processor)
        from .lmlogits import generate_with_cfg
        return generate_with_cfg(self, llm, batch_input_ids, batch_attention_mask, max_new_tokens, temperature, cfg_scale, top_k, top_p,
                                 repetition_penalty, pad_token_id, streamer, constrained_processor)

    # ------------------------------------------------------------------ B songs in one loop (opt-in)
    # The reference's pt backend generates the codes of a batch one song after the other (``_run_pt``, llm_inference.py:986-1070), and
    # its only batch caller passes the same prompt B times with B seeds (:1314-1373).  With ``use_native_lm_batch`` (ACE355_LM_BATCH=1
    # for every host) such a call runs as ace355.lmlogits.generate_codes_batch: one prefill of the CFG pair, the cache fanned out to B
    # + B sequences, one decode loop for all songs.  The flag implies the native loop and the native selection whatever their own
    # flags say.  Song i comes out token for token as the sequential native loop produces it for seeds[i] - not as
    # torch.multinomial would draw it - and the global RNG is left alone, where the reference leaves it seeded with the last item's
    # seed.  Every other call (lmlogits.batch_request says which, and why) goes to the host's ``_run_pt`` unchanged, the reason logged
    # once per handler (``[native-lm-batch] ...``); so does a call whose native part raises, which is safe because each sequential
    # item resets the processor.
    use_native_lm_batch: bool = _LM_BATCH_ENV
    _lm_batch_reasons_logged = frozenset()

    def _lm_batch_skip(self, why):
        if why not in self._lm_batch_reasons_logged:   # once per reason and handler
            self._lm_batch_reasons_logged = self._lm_batch_reasons_logged | {why}
            logger.info("[native-lm-batch] %s; this request runs item by item", why)

    def _run_pt_batch(self, prompt, n_items, seeds, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                      use_constrained_decoding, constrained_decoding_debug, target_duration, generation_phase, caption, lyrics, cot_text):
        """What ``_run_pt`` and ``_run_pt_single`` do around the loop, for ``n_items`` songs with one prompt: the list of their texts,
        or None (reason logged) when the tokenised pair does not fit the native handle."""
        from .lmlogits import batch_request, generate_codes_batch
        tok = self.llm_tokenizer
        texts = []
        with self._load_model_context():
            max_new_tokens = self._compute_max_new_tokens(target_duration=target_duration, generation_phase=generation_phase,
                                                          fallback_max=getattr(getattr(self.llm, "config", None), "max_new_tokens", 4096))
            uncond = self._build_unconditional_prompt(caption=caption, lyrics=lyrics, cot_text=cot_text, negative_prompt=negative_prompt,
                                                      generation_phase=generation_phase, is_batch=False)
            side = tok.padding_side
            tok.padding_side = "left"
            try:
                pair = tok([prompt, uncond], return_tensors="pt", padding=True, truncation=True)
            finally:
                tok.padding_side = side
            pair = {k: v.to(self.device) for k, v in pair.items()}
            ids, mask = pair["input_ids"], pair.get("attention_mask", None)
            llm, why = self._lm_loop_accepts(ids, mask, max_new_tokens)
            ok, why = batch_request([prompt] * n_items, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds,
                                    loop_refusal=why if llm is None else None)
            if not ok:
                self._lm_batch_skip(why)
                return None
            group = max(llm.max_seqs // 2, 1)
            for i0 in range(0, n_items, group):
                proc = self._setup_constrained_processor(
                    use_constrained_decoding=use_constrained_decoding, constrained_decoding_debug=constrained_decoding_debug,
                    target_duration=target_duration, user_metadata=None, stop_at_reasoning=False, skip_genres=True, skip_caption=True,
                    skip_language=True, generation_phase=generation_phase, is_batch=False)
                out = generate_codes_batch(self, llm, ids, mask, list(seeds[i0:min(i0 + group, n_items)]), max_new_tokens, temperature,
                                           cfg_scale, top_k, top_p, repetition_penalty, tok.pad_token_id or tok.eos_token_id, proc)
                new = out[:, ids.shape[1]:].cpu()
                texts += [tok.decode(row, skip_special_tokens=False) for row in new]
        return texts

    def _run_pt(self, formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                use_constrained_decoding=True, constrained_decoding_debug=False, target_duration=None, user_metadata=None,
                stop_at_reasoning=False, skip_genres=True, skip_caption=False, skip_language=False, generation_phase="cot", caption="",
                lyrics="", cot_text="", seeds=None):
        def sequential():
            return super(NativeLmMixin, self)._run_pt(
                formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                use_constrained_decoding=use_constrained_decoding, constrained_decoding_debug=constrained_decoding_debug,
                target_duration=target_duration, user_metadata=user_metadata, stop_at_reasoning=stop_at_reasoning,
                skip_genres=skip_genres, skip_caption=skip_caption, skip_language=skip_language, generation_phase=generation_phase,
                caption=caption, lyrics=lyrics, cot_text=cot_text, seeds=seeds)

        if self.use_native_lm_nocfg and not cfg_scale > 1.0:   # (a CFG request is none of this flag's)
            from .lmlogits import nocfg_batch_request
            ok, why = nocfg_batch_request(formatted_prompts, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds)
            texts = None
            if not ok:
                if isinstance(formatted_prompts, list) and len(formatted_prompts) > 1:   # a single prompt is no batch: nothing to say
                    self._lm_nocfg_skip(why, "this request runs item by item")
            else:
                try:
                    texts = self._run_pt_batch_nocfg(formatted_prompts[0], len(formatted_prompts), seeds, temperature, cfg_scale, top_k,
                                                     top_p, repetition_penalty, use_constrained_decoding, constrained_decoding_debug,
                                                     target_duration, generation_phase)
                except Exception as exc:
                    logger.warning("[native-lm-nocfg] %s: %s; this request runs item by item", type(exc).__name__, exc)
            if texts is not None:
                return texts
        if not self.use_native_lm_batch:
            return sequential()
        from .lmlogits import batch_request
        ok, why = batch_request(formatted_prompts, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds)
        if not ok:
            self._lm_batch_skip(why)
            return sequential()
        try:
            texts = self._run_pt_batch(formatted_prompts[0], len(formatted_prompts), seeds, temperature, cfg_scale, negative_prompt, top_k,
                                       top_p, repetition_penalty, use_constrained_decoding, constrained_decoding_debug, target_duration,
                                       generation_phase, caption, lyrics, cot_text)
        except Exception as exc:
            logger.warning("[native-lm-batch] %s: %s; this request runs item by item", type(exc).__name__, exc)
            texts = None
        return texts if texts is not None else sequential()

    # ------------------------------------------------------------------ the loop without CFG (opt-in)
    # The other half of ``_run_pt_single`` (llm_inference.py:929-942): with ``cfg_scale <= 1`` and constrained decoding it calls
    # ``_generate_with_constrained_decoding`` (:2321-2412) - every "understand"-phase request (understand_audio_from_codes,
    # create_sample_from_query, format_sample_from_input) and every codes request at lm_cfg_scale 1.0.  With ``use_native_lm_nocfg``
    # (ACE355_LM_NOCFG=1 for every host) that method is ace355.lmlogits.generate_constrained: the loop above with B sequences and no
    # unconditional rows, its stage in the model's dtype because that loop never upcasts (include/ace355.h, ace355_lm_shape_as).  A
    # ``_run_pt`` batch of one prompt with B seeds and ``cfg_scale <= 1`` runs as generate_codes_batch_nocfg, up to max_seqs songs
    # per loop.  The flag implies the native selection for these calls whatever the other flags say: the distribution is the
    # reference's, the draw for a seed is ace355.lmsample's.  Goes to the host's own method, the reason logged once per handler
    # (``[native-lm-nocfg] ...``): whatever ``_lm_loop_accepts`` refuses (not the native swap, ids not on the GPU, not left-padded,
    # B > max_seqs, P + max_new_tokens > max_positions, ...), and an fp16 ``out_dtype``.  The metadata FSM stays the reference's
    # code (run on the native forward's logits in the model's dtype), and ``llm.generate()`` without constrained decoding stays on
    # the kept module.
    use_native_lm_nocfg: bool = _LM_NOCFG_ENV
    _lm_nocfg_reasons_logged = frozenset()

    def _lm_nocfg_skip(self, why, then="this request runs the reference's loop"):
        if why not in self._lm_nocfg_reasons_logged:   # once per reason and handler
            self._lm_nocfg_reasons_logged = self._lm_nocfg_reasons_logged | {why}
            logger.info("[native-lm-nocfg] %s; %s", why, then)

    def _lm_nocfg_accepts(self, input_ids, attention_mask, max_new_tokens):
        """``_lm_loop_accepts`` for B >= 1 rows without unconditional ones, plus the dtypes the stage runs in."""
        llm, why = self._lm_loop_accepts(input_ids, attention_mask, max_new_tokens, pairs=False)
        if llm is not None and llm.out_dtype not in (torch.float32, torch.bfloat16):
            return None, f"the native LM's out_dtype {llm.out_dtype} is neither fp32 nor bf16"
        return llm, why

    def _generate_with_constrained_decoding(self, input_ids, attention_mask, max_new_tokens, temperature, top_k, top_p,
                                            repetition_penalty, pad_token_id, streamer, constrained_processor=None):
        llm = None
        if self.use_native_lm_nocfg:
            llm, why = self._lm_nocfg_accepts(input_ids, attention_mask, max_new_tokens)
            if llm is None:
                self._lm_nocfg_skip(why)
        if llm is None:
            return super()._generate_with_constrained_decoding(input_ids, attention_mask, max_new_tokens, temperature, top_k, top_p,
                                                               repetition_penalty, pad_token_id, streamer, constrained_processor)
        from .lmlogits import generate_constrained
        return generate_constrained(self, llm, input_ids, attention_mask, max_new_tokens, temperature, top_k, top_p, repetition_penalty,
                                    pad_token_id, streamer, constrained_processor)

    def _run_pt_batch_nocfg(self, prompt, n_items, seeds, temperature, cfg_scale, top_k, top_p, repetition_penalty,
                            use_constrained_decoding, constrained_decoding_debug, target_duration, generation_phase):
        """``_run_pt_batch`` for the non-CFG branch of ``_run_pt_single``: one row, ``padding=False`` (llm_inference.py:889-894)."""
        from .lmlogits import generate_codes_batch_nocfg, nocfg_batch_request
        tok = self.llm_tokenizer
        texts = []
        with self._load_model_context():
            max_new_tokens = self._compute_max_new_tokens(target_duration=target_duration, generation_phase=generation_phase,
                                                          fallback_max=getattr(getattr(self.llm, "config", None), "max_new_tokens", 4096))
            one = tok(prompt, return_tensors="pt", padding=False, truncation=True)
            one = {k: v.to(self.device) for k, v in one.items()}
            ids, mask = one["input_ids"], one.get("attention_mask", None)
            llm, why = self._lm_nocfg_accepts(ids, mask, max_new_tokens)
            ok, why = nocfg_batch_request([prompt] * n_items, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds,
                                          loop_refusal=why if llm is None else None)
            if not ok:
                self._lm_nocfg_skip(why, "this request runs item by item")
                return None
            group = max(llm.max_seqs, 1)
            for i0 in range(0, n_items, group):
                proc = self._setup_constrained_processor(
                    use_constrained_decoding=use_constrained_decoding, constrained_decoding_debug=constrained_decoding_debug,
                    target_duration=target_duration, user_metadata=None, stop_at_reasoning=False, skip_genres=True, skip_caption=True,
                    skip_language=True, generation_phase=generation_phase, is_batch=False)
                out = generate_codes_batch_nocfg(self, llm, ids, mask, list(seeds[i0:min(i0 + group, n_items)]), max_new_tokens,
                                                 temperature, top_k, top_p, repetition_penalty, tok.pad_token_id or tok.eos_token_id, proc)
                new = out[:, ids.shape[1]:].cpu()
                texts += [tok.decode(row, skip_special_tokens=False) for row in new]
        return texts


class NativeAudioInMixin:
    """The three loaders of ``IoAudioMixin`` (acestep/core/generation/handler/io_audio.py:39-133) on the native input stage
    (ace355.audio_in): same signatures, same None-on-failure behaviour, but the tensor they return is already on ``self.device``, so
    ``tiled_encode`` takes it without a copy.  Required host attribute: ``device``.  Opt-in (``use_native_audio_in``, or
    ACE355_AUDIO_IN=1 for every host): off, each call goes to the host's own method further up the MRO, untouched.
    ``native_flac_decode`` (or ACE355_FLAC_GPU=1) matters only while ``use_native_audio_in`` is on: a FLAC file's frames are then
    decoded on the GPU, 16 to 24 bits per sample (``audio_in.decode_flac``), instead of by the host decoder, which stops at 16."""

    use_native_audio_in: bool = _AUDIO_IN_ENV
    native_flac_decode: bool = _FLAC_GPU_ENV

    def _native_load_audio(self, audio_file):
        """(wav fp32 [2, S] at 48 kHz on ``self.device``, max|wav|) of a WAV / FLAC file."""
        from .audio_in import load_stereo_48k
        return load_stereo_48k(audio_file, self.device, flac_on_gpu=self.native_flac_decode)

    def _native_audio_in(self, name: str, audio_file, reference: bool = False):
        parent = getattr(super(), name, None)
        if not self.use_native_audio_in:
            if parent is None:
                raise RuntimeError("no audio input backend available: use_native_audio_in is off and the host has no loader of its own")
            return parent(audio_file)
        if audio_file is None:   # (every loader of the reference: None in, None out)
            return None
        try:
            wav, peak = self._native_load_audio(audio_file)
            if not reference:
                return wav
            if peak < 1e-6:   # is_silence (memory_utils.py:19-21): all |x| < 1e-6
                return None
            from .audio_in import reference_segments
            return reference_segments(wav)
        except NotImplementedError as exc:   # a format, bit depth or rate the native stage does not take
            if parent is not None:
                logger.info("[%s] %s; the host's loader reads this file", name, exc)
                return parent(audio_file)
            logger.warning("[%s] %s, and the host has no loader of its own", name, exc)
            return None
        except (OSError, RuntimeError, ValueError) as exc:
            if reference:
                logger.warning("[process_reference_audio] Invalid or unsupported reference audio: %s", exc)
            else:
                logger.exception("[%s] Error processing audio", name)
            return None

    def process_target_audio(self, audio_file: Optional[str]) -> Optional[torch.Tensor]:
        """io_audio.py:39-61."""
        return self._native_audio_in("process_target_audio", audio_file)

    def process_reference_audio(self, audio_file: Optional[str]) -> Optional[torch.Tensor]:
        """io_audio.py:63-113: the 3 x 10 s cut of the clip, None for a silent one."""
        return self._native_audio_in("process_reference_audio", audio_file, reference=True)

    def process_src_audio(self, audio_file: Optional[str]) -> Optional[torch.Tensor]:
        """io_audio.py:115-133."""
        return self._native_audio_in("process_src_audio", audio_file)


class _ModelShell:
    """What the mixins read from ``self.model``: decoder state dict, null embedding, config."""

    class _Dec:
        def __init__(self, sd):
            self._sd = sd

        def state_dict(self):
            return self._sd

    def __init__(self, cfg: DitConfig, decoder_sd: Dict[str, torch.Tensor], null_condition_emb: torch.Tensor):
        self.config = cfg
        self.decoder = self._Dec(decoder_sd)
        self.null_condition_emb = null_condition_emb


class NativeHandler(NativeDitMixin, NativeVaeMixin, NativeTextEncoderMixin, NativeAudioInMixin):
    """Self-contained counterpart of ``AceStepHandler`` for the denoise + decode path.

    Differences from the reference handler are confined to what is out of scope: conditioning arrives pre-embedded
    (``encoder_hidden_states``, ``context_latents``) instead of captions/lyrics; there is no LM phase.
    """

    sample_rate = 48000  # acestep/handler.py:120

    def __init__(self):
        self.model = None
        self.vae = None
        self.text_encoder = None
        self.device = "cpu"
        self.dtype = torch.float32
        self.use_lora = False
        self.quantization = None
        self.offload_to_cpu = False
        self.current_offload_cost = 0.0
        self.model_variant = "sft"  # which checkpoint family's generate_audio semantics apply: "base" | "sft" | "turbo"
        # data-parallel requests run in the library's launch-shape-independent mode (`shape_independent` below): a song's bits then do
        # not depend on how many ranks share the request.  False: the default (fastest) launch policy, batch-dependent low bits.
        self.dp_shape_independent = True
        # LoRA registry (the reference's H/lora/lifecycle.py / controls.py state): adapter name -> its terms (PEFT scaling, device bf16)
        self.lora_loaded = False
        self.lora_scale = 1.0
        self._lora_registry: Dict[str, list] = {}
        self._active_loras: Dict[str, float] = {}
        self._lora_active_adapter: Optional[str] = None
        self._adapter_type: Optional[str] = None   # "lora" | "lokr" (lifecycle.py:236, 242)
        from .align import DEFAULT_LAYERS_HEADS
        self.custom_layers_config = {k: list(v) for k, v in DEFAULT_LAYERS_HEADS.items()}   # acestep/handler.py:129

    def initialize_service(self, dit_config: DitConfig, decoder_state_dict: Dict[str, torch.Tensor],
                           null_condition_emb: torch.Tensor, vae_config: Optional[VaeConfig] = None,
                           vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, device: str = "auto",
                           use_native: bool = True, model_variant: str = "sft",
                           text_encoder_config: Optional[TextEncoderConfig] = None,
                           text_encoder_state_dict: Optional[Dict[str, torch.Tensor]] = None):
        """Counterpart of ``initialize_service`` (handler/init_service_orchestrator.py:15-110) for pre-loaded weights.
        Re-entry is allowed (:30-31).  Returns ``(status_message, success)`` like the reference.
        ``text_encoder_config`` + ``text_encoder_state_dict`` (``Qwen3Model.state_dict()`` keys): the handler also gets
        ``text_encoder`` (a ``NativeTextEncoder``) and the reference's ``infer_text_embeddings`` / ``infer_lyric_embeddings`` work.
        ``model_variant`` names the checkpoint family (the reference reads it off the checkpoint directory,
        handler/init_service_catalog.py:69-73): "base" ignores explicit ``timesteps`` like its model, "sft" honours them,
        "turbo" selects the 8-step table sampler without CFG."""
        try:
            if model_variant not in ("base", "sft", "turbo"):
                raise ValueError(f"unknown model_variant '{model_variant}'")
            self.model_variant = model_variant
            if device == "auto":
                device = "cuda" if torch.cuda.is_available() else "cpu"
            if device == "cuda":
                device = f"cuda:{torch.cuda.current_device()}"
            self.device = device
            self.dtype = torch.bfloat16 if str(device).startswith("cuda") else torch.float32  # orchestrator :51
            self.model = _ModelShell(dit_config, decoder_state_dict, null_condition_emb)
            self.vae_config, self.vae_state_dict = vae_config, vae_state_dict
            if not use_native:
                return "native backend disabled", False
            if not str(device).startswith("cuda"):
                raise RuntimeError("the native backend needs a ROCm GPU (no CPU fallback)")
            ok = self._init_native_dit()
            if ok and vae_state_dict is not None:
                ok = self._init_native_vae()
            if ok and (text_encoder_config is not None or text_encoder_state_dict is not None):
                if text_encoder_config is None or text_encoder_state_dict is None:
                    raise ValueError("text_encoder_config and text_encoder_state_dict go together")
                from .textenc import NativeTextEncoder
                self.text_encoder = None
                te = NativeTextEncoder(text_encoder_config, device, out_dtype=self.dtype)
                te.load_state_dict(text_encoder_state_dict)
                self.text_encoder, self.use_native_text_encoder = te, True
            return ("native backend ready" if ok else "native backend failed to initialise"), bool(ok)
        except Exception as exc:
            logger.exception("initialize_service failed")
            return f"Error: {exc!s}", False

    # ------------------------------------------------------------------ text encoder (conditioning_embed.py:71-79)
    def infer_text_embeddings(self, text_token_idss):
        """Infer text-token embeddings via text encoder."""
        with torch.inference_mode():
            return self.text_encoder(input_ids=text_token_idss, lyric_attention_mask=None).last_hidden_state

    def infer_lyric_embeddings(self, lyric_token_ids):
        """Infer lyric-token embeddings via text encoder embedding table."""
        with torch.inference_mode():
            return self.text_encoder.embed_tokens(lyric_token_ids)

    # ------------------------------------------------------------------ LoRA (H/lora/lifecycle.py, H/lora/controls.py)
    def add_lora(self, lora_path: str, adapter_name: Optional[str] = None) -> str:
        """Load the PEFT LoRA directory or LoKr artefact ``lora_path`` as ``adapter_name`` (default: the path's last component) and make
        it the active adapter (lifecycle.py:164-286).  The native DiT merges it at the next request (``_sync_native_adapters``)."""
        import os
        from .dora import DoraTerm
        from .lokr import read_lokr_adapter, resolve_lokr_weights_path
        from .lora import read_peft_adapter
        if self.model is None:
            return "❌ Model not initialized. Please initialize service first."
        if self.quantization is not None:
            return ("❌ LoRA loading is not supported on quantized models. "
                    f"Current quantization: {self.quantization}. "
                    "Please re-initialize the service with quantization disabled, then try loading the LoRA adapter again.")
        if not lora_path or not lora_path.strip():
            return "❌ Please provide a LoRA path."
        lora_path = lora_path.strip()
        if not os.path.exists(lora_path):
            return f"❌ LoRA path not found: {lora_path}"
        name = adapter_name.strip() if isinstance(adapter_name, str) and adapter_name.strip() else \
            (os.path.basename(lora_path.rstrip(os.sep)) or "default")
        if name in self._lora_registry:
            return f"❌ Adapter name already in use: {name}. Use a different name or remove it first."
        lokr_path = resolve_lokr_weights_path(lora_path)
        if self._lora_registry and lokr_path is not None and self._adapter_type != "lokr":   # lifecycle.py:244-246
            return "❌ LoKr cannot be added as a second adapter when PEFT is already loaded."
        if self._lora_registry and self._adapter_type == "lokr":
            return "❌ A LoKr adapter is loaded; unload it before loading another adapter."
        try:
            dev = torch.device(self.device)
            if lokr_path is not None:
                logger.info("Loading LoKr adapter from %s as '%s'", lokr_path, name)
                terms = read_lokr_adapter(lokr_path, self.model.config, allow_dora=True, dtype=self.dtype)
                self._lora_registry[name] = [t if isinstance(t, DoraTerm) else
                                             t._replace(**{f: getattr(t, f).to(dev, self.dtype) for f in t._fields[1:7]
                                                           if getattr(t, f) is not None}) for t in terms]
            else:
                terms = read_peft_adapter(lora_path, self.model.config, allow_dora=True)
                self._lora_registry[name] = [t if isinstance(t, DoraTerm) else
                                             t._replace(A=t.A.to(dev, self.dtype), B=t.B.to(dev, self.dtype)) for t in terms]
            # DoRA magnitudes: the values the reference holds after its cast to the model dtype, as the fp32 the merge reads
            self._lora_registry[name] = [t._replace(g=t.g.to(dev, self.dtype).float().reshape(-1).contiguous())
                                         if isinstance(t, DoraTerm) else t for t in self._lora_registry[name]]
        except Exception as exc:
            logger.exception("Failed to load LoRA adapter")
            return f"❌ Failed to load LoRA: {exc!s}"
        self._adapter_type = "lokr" if lokr_path is not None else "lora"
        self.lora_loaded = True
        self.use_lora = True
        self._active_loras[name] = 1.0
        self._lora_active_adapter = name
        return f"✅ LoRA '{name}' loaded from {lora_path}"

    def load_lora(self, lora_path: str) -> str:
        """Single-adapter form of ``add_lora`` (lifecycle.py:289-295)."""
        from .lokr import resolve_lokr_weights_path
        lokr_path = resolve_lokr_weights_path(lora_path.strip()) if isinstance(lora_path, str) else None
        message = self.add_lora(lora_path, adapter_name=None)
        if lokr_path is not None and message.startswith("✅"):
            return f"✅ LoKr loaded from {lokr_path}"
        return message

    def remove_lora(self, adapter_name: str) -> str:
        if not self._lora_registry:
            return "⚠️ No LoRA adapter loaded."
        if adapter_name not in self._lora_registry:
            return f"❌ Unknown adapter: {adapter_name}. Loaded: {list(self._lora_registry.keys())}"
        del self._lora_registry[adapter_name]
        self._active_loras.pop(adapter_name, None)
        if not self._lora_registry:
            return self._lora_reset()
        if self._lora_active_adapter == adapter_name:
            self._lora_active_adapter = next(iter(self._lora_registry))
        return f"✅ Adapter '{adapter_name}' removed. Active: {self._lora_active_adapter}"

    def unload_lora(self) -> str:
        if not self._lora_registry:
            return "⚠️ No LoRA adapter loaded."
        return self._lora_reset()

    def _lora_reset(self) -> str:
        self._lora_registry.clear()
        self._active_loras.clear()
        self._lora_active_adapter = None
        self.lora_loaded = False
        self.use_lora = False
        self._adapter_type = None
        self.lora_scale = 1.0
        return "✅ LoRA unloaded, using base model"

    def set_use_lora(self, use_lora: bool) -> str:
        """controls.py:35-80."""
        if use_lora and not self.lora_loaded:
            return "❌ No LoRA adapter loaded. Please load a LoRA first."
        self.use_lora = bool(use_lora)
        return f"✅ {self._adapter_label()} {'enabled' if use_lora else 'disabled'}"

    def set_lora_scale(self, adapter_name_or_scale, scale: Optional[float] = None) -> str:
        """Scale of one adapter, clamped to [0, 1] (controls.py:83-113): ``set_lora_scale(0.5)`` for the active adapter or
        ``set_lora_scale(name, 0.5)``."""
        import math
        if not self.lora_loaded:
            return "⚠️ No LoRA loaded"
        if scale is None:
            value, name = adapter_name_or_scale, None
        else:
            value, name = scale, adapter_name_or_scale if isinstance(adapter_name_or_scale, str) else None
        try:
            value = float(value)
        except (TypeError, ValueError):
            return "❌ Invalid LoRA scale: please provide a numeric value between 0 and 1."
        if not math.isfinite(value):
            return "❌ Invalid LoRA scale: please provide a finite numeric value between 0 and 1."
        value = max(0.0, min(1.0, value))
        name = name or self._lora_active_adapter or next(iter(self._active_loras), None)
        if not name:
            return "❌ No adapter specified and no active adapter. Load a LoRA or pass adapter_name."
        if name not in self._lora_registry:
            return f"❌ Adapter '{name}' not in loaded adapters: {list(self._lora_registry.keys())}"
        self._active_loras[name] = value
        self.lora_scale = value
        label = self._adapter_label()   # (controls.py:115-127)
        if not self.use_lora:
            return f"✅ {label} scale ({name}): {value:.2f} ({label} disabled)"
        return f"✅ {label} scale ({name}): {value:.2f}"

    def set_active_lora_adapter(self, adapter_name: str) -> str:
        """Only the active adapter applies (PEFT's set_adapter; controls.py:193-205)."""
        if adapter_name not in self._lora_registry:
            return f"❌ Unknown adapter: {adapter_name}"
        self._lora_active_adapter = adapter_name
        return f"✅ Active LoRA adapter: {adapter_name}"

    def _adapter_label(self) -> str:
        return "LoKr" if self._adapter_type == "lokr" else "LoRA"   # (controls.py:78)

    def get_lora_status(self) -> Dict[str, Any]:
        return {"loaded": self.lora_loaded, "active": self.use_lora, "scale": self.lora_scale, "scales": dict(self._active_loras),
                "active_adapter": self._lora_active_adapter, "adapters": list(self._lora_registry.keys()),
                "adapter_type": self._adapter_type, "label": self._adapter_label()}

    def _native_adapter_terms(self):
        """The active adapter of this handler's registry, at its scale."""
        name = self._lora_active_adapter
        if not name or name not in self._lora_registry:
            return []
        s = float(self._active_loras.get(name, 1.0))
        # a DoRA term's scale is the m of its interpolation: LyCORIS' multiplier (the user's scale, controls.py:12-32) enters it, PEFT's
        # scaling does not
        return [t if hasattr(t, "per_input") and self._adapter_type != "lokr" else t._replace(scale=t.scale * s)
                for t in self._lora_registry[name]]

    # ------------------------------------------------------------------ service_generate
    def service_generate(self, encoder_hidden_states: torch.Tensor, context_latents: torch.Tensor,
                         src_latents: Optional[torch.Tensor] = None, seed: Union[int, List[int], None] = None,
                         infer_steps: int = 30, guidance_scale: float = 7.0, audio_cover_strength: float = 1.0,
                         cover_noise_strength: float = 0.0, infer_method: str = "ode", use_adg: bool = False,
                         cfg_interval_start: float = 0.0, cfg_interval_end: float = 1.0, shift: float = 1.0,
                         timesteps: Optional[Sequence[float]] = None, encoder_hidden_states_non_cover=None,
                         context_latents_non_cover=None) -> Dict[str, Any]:
        """The diffusion half of ``service_generate`` (handler/service_generate.py:21-146) from prepared conditions."""
        B = context_latents.shape[0]
        if B > MAX_BATCH_SIZE:  # handler/service_generate_request.py:66-75 clamps; we refuse explicitly
            raise ValueError(f"batch size {B} exceeds the per-call cap of {MAX_BATCH_SIZE}")
        if src_latents is None:
            src_latents = context_latents[..., : context_latents.shape[-1] // 2]
        with torch.inference_mode():
            outputs = self._native_run_diffusion(
                encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=None, context_latents=context_latents,
                src_latents=src_latents, seed=seed, infer_method=infer_method, shift=shift, timesteps=timesteps,
                audio_cover_strength=audio_cover_strength, encoder_hidden_states_non_cover=encoder_hidden_states_non_cover,
                context_latents_non_cover=context_latents_non_cover, infer_steps=infer_steps, guidance_scale=guidance_scale,
                cfg_interval_start=cfg_interval_start, cfg_interval_end=cfg_interval_end, use_adg=use_adg,
                cover_noise_strength=cover_noise_strength)
        outputs.update({"src_latents": src_latents, "encoder_hidden_states": encoder_hidden_states,
                        "context_latents": context_latents, "encoder_attention_mask": None})
        return outputs

    # ------------------------------------------------------------------ generate_music
    def generate_music(self, encoder_hidden_states: Optional[torch.Tensor], context_latents: Optional[torch.Tensor], seed=None,
                       inference_steps: int = 27, guidance_scale: float = 7.0, shift: float = 1.0, infer_method: str = "ode",
                       timesteps=None, use_tiled_decode: bool = True, latent_shift: float = 0.0, latent_rescale: float = 1.0,
                       cfg_interval_start: float = 0.0, cfg_interval_end: float = 1.0, use_adg: bool = False,
                       progress=None, data_parallel: bool = False, **service_kwargs) -> Dict[str, Any]:
        """Counterpart of ``AceStepHandler.generate_music`` (handler/generate_music.py:22-190) from prepared conditions.
        Never raises: every exception becomes the reference's error payload.

        ``data_parallel=True`` inside an initialised ``torch.distributed`` group (one process per GPU, every rank holding an
        initialised handler): rank 0 passes the request of G songs (one seed per song), the other ranks pass ``None`` tensors;
        the request is broadcast once, each rank generates its contiguous slice (``ace355.dist.run_request``: 8/4/2/1 songs
        per rank for a batch of 8 on 1/2/4/8 GPUs) and rank 0 returns the payload with all G songs in order (the other ranks
        return theirs).  Every per-request setting (steps, guidance, shift, CFG interval, ADG, ode / sde, explicit timesteps, tiled
        decode, latent shift / rescale, cover strength / cover noise strength) is rank 0's and travels with the request, and so do a cover
        request's tensors (``src_latents``, ``encoder_hidden_states_non_cover``, ``context_latents_non_cover`` in ``service_kwargs``);
        any other keyword is refused on every rank.  A song's noise, schedule and conditions never depend on the rank or the batch it
        runs in; by default (``self.dp_shape_independent = True``) neither do its bits: the request runs inside ``shape_independent()`` (one K order,
        no split-K / split-KV, one sampler chain), so rank 0's G songs equal a single-process call of the same request under the same mode bit
        for bit (tests/test_dist_gpu.py).  With ``dp_shape_independent = False`` every rank keeps the fastest launch policy for ITS slice and the
        low bits follow the slice size (~3e-3 relative L2, both at the reference's distance); the payload says which:
        ``extra_outputs["data_parallel"]["batch_dependent_bits"]``.  ``extra_outputs`` (pred_latents, src_latents, ...)
        describe the RETURNING rank's slice ``extra_outputs["song_range"]``, ``audios`` on rank 0 all G songs.  The per-call cap of 8 (handler/service_generate_request.py:12) then holds per rank."""
        if data_parallel and self.use_lora and self._native_adapter_terms():
            # adapters live in this process's registry only: they are not part of the broadcast request
            return self._error_payload(RuntimeError("data_parallel: LoRA adapters are rank-local and not part of the broadcast request; "
                                                    "disable or remove the adapter first"))
        if data_parallel:
            import torch.distributed as dist
            if dist.is_initialized() and dist.get_world_size() > 1:
                return self._generate_music_data_parallel(
                    encoder_hidden_states, context_latents, seed, progress,
                    dict(inference_steps=inference_steps, guidance_scale=guidance_scale, shift=shift, cfg_interval_start=cfg_interval_start,
                         cfg_interval_end=cfg_interval_end, use_adg=float(bool(use_adg)), infer_method_sde=float(infer_method == "sde")),
                    dict(timesteps=timesteps, use_tiled_decode=use_tiled_decode, latent_shift=latent_shift, latent_rescale=latent_rescale,
                         **service_kwargs))
        try:
            payload, _ = self._generate_music_local(encoder_hidden_states, context_latents, seed, inference_steps, guidance_scale, shift,
                                                    infer_method, timesteps, use_tiled_decode, latent_shift, latent_rescale,
                                                    cfg_interval_start, cfg_interval_end, use_adg, progress, service_kwargs)
            return payload
        except Exception as exc:  # handler/generate_music.py:181-190
            return self._error_payload(exc)

    @staticmethod
    def _error_payload(exc) -> Dict[str, Any]:
        logger.exception("[generate_music] Generation failed")
        return {"audios": [], "status_message": f"Error: {exc!s}\n{traceback.format_exc()}", "extra_outputs": {},
                "success": False, "error": f"{exc!s}"}

    def _generate_music_local(self, encoder_hidden_states, context_latents, seed, inference_steps, guidance_scale, shift, infer_method,
                              timesteps, use_tiled_decode, latent_shift, latent_rescale, cfg_interval_start, cfg_interval_end, use_adg,
                              progress, service_kwargs):
        """The single-GPU body: service_generate -> _prepare_decode_state -> tiled_decode -> peak normalise -> payload.
        Returns (payload, waveforms on the device [B, 2, samples]); raises on failure."""
        if progress:
            progress(0.52, desc="Generating music...")
        outputs = self.service_generate(encoder_hidden_states, context_latents, seed=seed, infer_steps=inference_steps,
                                        guidance_scale=guidance_scale, shift=shift, infer_method=infer_method,
                                        timesteps=timesteps, cfg_interval_start=cfg_interval_start,
                                        cfg_interval_end=cfg_interval_end, use_adg=use_adg, **service_kwargs)
        pred_latents, time_costs = self._prepare_decode_state(outputs, latent_shift, latent_rescale)
        if progress:
            progress(0.8, desc="Decoding audio...")
        t0 = time.time()
        with torch.inference_mode():
            pred_latents_cpu = pred_latents.detach().cpu()
            z = pred_latents.transpose(1, 2).contiguous()  # handler/generate_music_decode.py:123
            pred_wavs = self.tiled_decode(z) if use_tiled_decode else self._native_vae_decode(z)
            if pred_wavs.dtype != torch.float32:
                pred_wavs = pred_wavs.float()
            if pred_wavs.is_cuda:
                from .vae import peak_normalize
                pred_wavs = peak_normalize(pred_wavs.contiguous())
            else:
                peak = pred_wavs.abs().amax(dim=[1, 2], keepdim=True)
                if torch.any(peak > 1.0):
                    pred_wavs = pred_wavs / peak.clamp(min=1.0)
            if pred_wavs.is_cuda:
                torch.cuda.synchronize(pred_wavs.device)
        time_costs["vae_decode_time_cost"] = time.time() - t0
        time_costs["total_time_cost"] = time_costs["total_time_cost"] + time_costs["vae_decode_time_cost"]
        time_costs["offload_time_cost"] = self.current_offload_cost
        B = pred_wavs.shape[0]
        audios = [{"tensor": pred_wavs[i].cpu(), "sample_rate": self.sample_rate} for i in range(B)]
        seed_value = seed[0] if isinstance(seed, (list, tuple)) and seed else seed
        extra = {"pred_latents": pred_latents_cpu, "target_latents": None,
                 "src_latents": outputs["src_latents"].detach().cpu(), "chunk_masks": None, "latent_masks": None, "spans": [],
                 "time_costs": time_costs, "seed_value": seed_value,
                 "encoder_hidden_states": outputs["encoder_hidden_states"].detach().cpu(), "encoder_attention_mask": None,
                 "context_latents": outputs["context_latents"].detach().cpu(), "lyric_token_idss": None}
        return ({"audios": audios, "status_message": "Generation completed successfully!", "extra_outputs": extra,
                 "success": True, "error": None}, pred_wavs)

    def _generate_music_data_parallel(self, encoder_hidden_states, context_latents, seed, progress, knobs, local_kwargs) -> Dict[str, Any]:
        """One request over every rank of the process group (``ace355.dist.run_request``).  A failure on ANY rank becomes the error
        payload on EVERY rank: the ranks agree on success (one MAX all-reduce) before the gather, so nobody waits in a
        collective the failed rank never joins."""
        import torch.distributed as dist
        from . import dist as a_dist
        rank, world = dist.get_rank(), dist.get_world_size()
        err: Optional[BaseException] = None
        request = None
        state: Dict[str, Any] = {}
        try:
            if rank == 0:
                if encoder_hidden_states is None or context_latents is None:
                    raise ValueError("data_parallel: rank 0 must pass the request tensors")
                G = max(encoder_hidden_states.shape[0], context_latents.shape[0])
                if not isinstance(seed, (list, tuple)) or len(seed) != G or any(s is None or int(s) < 0 for s in seed):
                    raise ValueError("data_parallel: one explicit seed per song is required (per-item generators make a song's NOISE "
                                     "independent of the rank and batch it runs in; a scalar seed couples the batch, base.py:1733-1770)")
                if G > MAX_BATCH_SIZE * world:
                    raise ValueError(f"batch size {G} exceeds the per-call cap of {MAX_BATCH_SIZE} on {world} ranks")
                shipped = ("timesteps", "use_tiled_decode", "latent_shift", "latent_rescale", "audio_cover_strength", "cover_noise_strength",
                           "src_latents", "encoder_hidden_states_non_cover", "context_latents_non_cover")
                extra = {kk: v for kk, v in local_kwargs.items() if kk not in shipped and v is not None}
                if extra:
                    # an argument that does not travel would apply on rank 0 only (advisor r3): refused on every rank rather than
                    # silently diverging.  Cover / repaint requests DO travel (round 5, advisor r4): strengths as knobs, tensors as items.
                    raise ValueError(f"data_parallel: these arguments are not part of the broadcast request: {sorted(extra)}")
                for kk in ("audio_cover_strength", "cover_noise_strength"):
                    if local_kwargs.get(kk) is not None:
                        knobs = dict(knobs, **{kk: float(local_kwargs[kk])})
                src_ship = local_kwargs.get("src_latents")
                if src_ship is None and float(local_kwargs.get("cover_noise_strength") or 0.0) > 0.0:
                    # the renoised start t x noise + (1 - t) x src is fp32 host arithmetic on the FULL-precision source half of the context; the
                    # context itself travels in bf16, so the default source is shipped explicitly (advisor r5: same bits as a single-GPU call)
                    src_ship = context_latents[..., : context_latents.shape[-1] // 2].float()
                request = a_dist.pack_request(encoder_hidden_states, context_latents, [int(s) for s in seed], None,
                                              timesteps=local_kwargs.get("timesteps"), use_tiled_decode=float(bool(local_kwargs.get("use_tiled_decode", True))),
                                              latent_shift=float(local_kwargs.get("latent_shift", 0.0)),
                                              latent_rescale=float(local_kwargs.get("latent_rescale", 1.0)),
                                              src_latents=src_ship,
                                              encoder_hidden_states_non_cover=local_kwargs.get("encoder_hidden_states_non_cover"),
                                              context_latents_non_cover=local_kwargs.get("context_latents_non_cover"), **knobs)
        except Exception as exc:
            err = exc
        # (rank 0 could not even build the request: the others learn it from an empty one)
        if rank == 0 and request is None:
            request = {"enc_rows": torch.zeros(0, 1, 1), "enc_index": torch.zeros(0, dtype=torch.int32), "ctx": torch.zeros(1, 1, 2),
                       "seeds": torch.zeros(0, dtype=torch.int64), "knobs": torch.zeros(len(a_dist.KNOBS), dtype=torch.float64),
                       "timesteps": torch.zeros(0)}

        def execute(local):
            k = local["knobs"]
            # every setting comes from the BROADCAST request (rank 0's call), none from this rank's own arguments
            state["shape_independent"] = bool(self.dp_shape_independent)
            with self.shape_independent(self.dp_shape_independent):
                payload, wavs = self._generate_music_local(
                    local["encoder_hidden_states"], local["context_latents"], local["seeds"], int(k["inference_steps"]), k["guidance_scale"],
                    k["shift"], "sde" if k["infer_method_sde"] else "ode", local["timesteps"], bool(k["use_tiled_decode"]),
                    k["latent_shift"], k["latent_rescale"], k["cfg_interval_start"], k["cfg_interval_end"],
                    bool(k["use_adg"]), progress if rank == 0 else None,
                    dict(audio_cover_strength=k["audio_cover_strength"], cover_noise_strength=k["cover_noise_strength"],
                         src_latents=local["src_latents"], encoder_hidden_states_non_cover=local["encoder_hidden_states_non_cover"],
                         context_latents_non_cover=local["context_latents_non_cover"]))
            state["payload"] = payload
            return wavs

        res = None
        try:
            res = a_dist.run_request(request, lambda local: self._dp_guard(execute, local, state), src=0, device=torch.device(self.device), gather=False)
        except Exception as exc:
            err = err or exc
        if err is None and "error" in state:
            err = state["error"]
        cdev = torch.device("cpu") if a_dist.host_staged() else torch.device(self.device)   # (gloo: collectives on host tensors)
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32, device=cdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()):
            return self._error_payload(err if err is not None else RuntimeError("generation failed on another rank"))
        wavs = res["local"]
        if wavs is None:   # this rank owns no song
            wavs = torch.empty(0, 2, 0, device=torch.device(self.device))
        # song-major gather to rank 0 (ace355.dist.gather_waveforms: sizes through one all_gather, payloads point to point)
        gathered = a_dist.gather_waveforms(wavs, dst=0)
        payload = state.get("payload") or {"audios": [], "status_message": "Generation completed successfully!", "extra_outputs": {},
                                           "success": True, "error": None}
        payload["extra_outputs"]["song_range"] = res["range"]
        if rank != 0:
            return payload
        audios = list(payload["audios"])
        for r in range(1, world):
            audios += [{"tensor": gathered[r][i].cpu(), "sample_rate": self.sample_rate} for i in range(gathered[r].shape[0])]
        payload["audios"] = audios
        payload["extra_outputs"]["data_parallel"] = {"world": world, "global_batch": res["global_batch"],
                                                     "batch_dependent_bits": not state.get("shape_independent", False)}
        return payload

    @contextlib.contextmanager
    def shape_independent(self, on: bool = True):
        """Run the enclosed native calls with ONE arithmetic per song whatever the launch shape: `ace355_gemm_set_k_rotation(0)` (no K
        rotation, no split-K, no split-KV / key-split attention: include/ace355.h) and one sampler chain (`ace355_dit_set_dual(0)`).  (The folded RMSNorms stay on: their
        row sums are gathered per aligned 128-column group in one fp32 order whatever the GEMM tile)  A song
        generated alone, inside a batch of 8, or on any rank of a data-parallel request then comes out bit for bit the same
        (tests/test_dist_gpu.py, tests/test_metric_shapes_gpu.py).  Costs the small-request optimisations their gain (measured per
        request in DESIGN.md section 14); process-wide while active (the K-rotation mode is a library global)."""
        if not on or self.native_dit is None:
            yield
            return
        from . import native
        prev_k = native.gemm_set_k_rotation(0)
        prev_d = self.native_dit.set_dual(0)
        try:
            yield
        finally:
            native.gemm_set_k_rotation(prev_k)
            self.native_dit.set_dual(prev_d)

    @staticmethod
    def _dp_guard(execute, local, state):
        try:
            return execute(local)
        except Exception as exc:  # reported through the all-reduce of the caller, not raised past the collectives
            state["error"] = exc
            return None

    def _prepare_decode_state(self, outputs: Dict[str, Any], latent_shift: float, latent_rescale: float):
        """handler/generate_music_decode.py:16-96: NaN/Inf and all-zero guards, latent * rescale + shift."""
        pred = outputs["target_latents"]
        time_costs = outputs["time_costs"]
        time_costs["offload_time_cost"] = self.current_offload_cost
        if pred.is_cuda:
            from .vae import latent_check
            bad, zero = latent_check(pred)
        else:
            bad = bool(torch.isnan(pred).any() or torch.isinf(pred).any())
            zero = bool(pred.numel() > 0 and pred.abs().sum() == 0)
        if bad:
            raise RuntimeError("Generation produced NaN or Inf latents. This usually indicates a checkpoint/config mismatch "
                               "or unsupported quantization/backend combination.")
        if zero:
            raise RuntimeError("Generation produced zero latents. This usually indicates a checkpoint/config mismatch or unsupported setup.")
        if latent_shift != 0.0 or latent_rescale != 1.0:
            pred = pred * latent_rescale + latent_shift
        return pred.float(), time_costs
