"""The reference's LM quality score (``acestep/core/scoring/lm_score.py``) on the native 5 Hz LM.

The reference scores a generation by teacher forcing: for every condition (six metadata fields, the caption, the lyrics) it runs the
LM over ``prompt + target``, copies the ``[T, V]`` logits of the target positions to the host, and takes a ``log_softmax`` (caption and
lyrics: mean log-probability, conditional minus unconditional = PMI) or a ``topk`` (metadata: position-weighted top-k recall) there.
All either needs per target token is one log-probability and one rank; ``NativeCausalLM.score`` (``ace355_lm_score``,
csrc/lm_score.hip) returns exactly those, and no logits leave the GPU.

This module carries the reference's entry points - same signatures, return values, status text and error strings - on top of
``target_stats``.  The UI imports ``calculate_pmi_score_per_condition`` from here in place of the reference's.

Routing.  The native path is taken when ``llm_handler.use_native_lm_score`` is set (``NativeLmMixin``; ``ACE355_LM_SCORE=1``),
``llm_handler.llm`` is the native swap or a bare ``NativeCausalLM``, and ``llm_backend`` is ``pt`` or absent.  Every other call, and any
call whose native path raises, runs the reference's own function when ``acestep.core.scoring.lm_score`` imports; a native failure is
logged under ``[native-lm-score]``, at most three times.  Without the reference, ``calculate_pmi_score_per_condition`` returns the
reference's error payload.

One difference is inherent: the reference's recall follows ``torch.topk``'s order among EQUAL logits, which is unspecified; here equal
logits are ordered by ascending id (a hit at k exists exactly when ``rank < k``), as the native token selection orders them.
"""
from __future__ import annotations

import contextlib
import logging
import math
from typing import Any, Dict, Optional, Tuple

import torch

logger = logging.getLogger("ace355")

RECALL_KEYS = ("bpm", "duration", "genres", "keyscale", "language", "timesignature")   # scored by top-k recall; the caption by PMI
_failures = 0


# ------------------------------------------------------------------------------------------------------------------ routing
def _reference():
    """The host's ``acestep.core.scoring.lm_score`` module, or None."""
    try:
        from acestep.core.scoring import lm_score
        return lm_score
    except Exception:
        return None


def native_lm(llm_handler):
    """The ``NativeCausalLM`` the native path would score with, or None when the routing rules send the call to the reference."""
    if not getattr(llm_handler, "use_native_lm_score", False):
        return None
    if getattr(llm_handler, "llm_backend", "pt") != "pt":
        return None
    from .lm import NativeCausalLM
    from .modswap import native_of
    llm = native_of(getattr(llm_handler, "llm", None))
    return llm if isinstance(llm, NativeCausalLM) else None


def _note_failure(exc: BaseException) -> None:
    global _failures
    _failures += 1
    if _failures <= 3:
        logger.warning("[native-lm-score] %s: %s; scoring this call with the reference's function", type(exc).__name__, exc)


def _routed(name: str, native_fn, llm_handler, *args, **kwargs):
    """``native_fn`` when the native path is taken and does not raise, else the reference's function ``name``; without the reference
    the native error (or a RuntimeError) propagates."""
    err: Optional[BaseException] = None
    if native_lm(llm_handler) is not None:
        try:
            return native_fn(llm_handler, *args, **kwargs)
        except Exception as exc:
            _note_failure(exc)
            err = exc
    ref = _reference()
    if ref is None:
        if err is not None:
            raise err
        raise RuntimeError(f"ace355.lmscore.{name}: the native path is not active and acestep.core.scoring.lm_score does not import")
    return getattr(ref, name)(llm_handler, *args, **kwargs)


# ------------------------------------------------------------------------------------------------------------------ native statistics
def score_rows(x: torch.Tensor, W: torch.Tensor, targets: torch.Tensor, row_index: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ace355_lm_score_rows`` on device tensors: ``x`` bf16 ``[M, D]`` (unit column stride, any row stride that is a multiple of 8),
    ``W`` bf16 ``[V, D]`` contiguous, ``targets`` int32 ``[R]``, ``row_index`` int32 ``[R]`` naming rows of ``x`` (None: rows 0 .. R - 1).
    Returns ``(logprob fp32 [R], rank int32 [R])`` on the device; no logits are stored."""
    from . import native
    if x.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or x.dim() != 2 or W.dim() != 2 or not x.is_cuda or W.device != x.device:
        raise ValueError("ace355: score_rows takes bf16 x [M, D] and W [V, D] on one GPU")
    if x.stride(1) != 1 or not W.is_contiguous() or x.shape[1] != W.shape[1]:
        raise ValueError("ace355: score_rows needs K-contiguous x and a contiguous W with the same D")
    for name, t in (("targets", targets), ("row_index", row_index)):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"ace355: score_rows {name} must be a contiguous int32 vector on {x.device}")
    R, (V, D) = int(targets.shape[0]), W.shape
    if row_index is not None and row_index.shape[0] != R:
        raise ValueError("ace355: score_rows row_index and targets differ in length")
    if row_index is None and R > x.shape[0]:
        raise ValueError(f"ace355: score_rows has {R} targets for {x.shape[0]} rows")
    nbytes = native.lm_score_workspace_bytes(R, V)
    if nbytes <= 0:
        raise ValueError(f"ace355: score_rows of {R} rows x {V} ids is outside the limits")
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        logprob = torch.empty(R, dtype=torch.float32, device=x.device)
        rank = torch.empty(R, dtype=torch.int32, device=x.device)
        native.check(native.lib().ace355_lm_score_rows(int(x.data_ptr()), int(x.stride(0)), native.ptr(row_index),
                                                       native.ptr(W), native.ptr(targets), R, int(V), int(D), native.ptr(logprob),
                                                       native.ptr(rank), native.ptr(ws), ws.numel(), native.current_stream_ptr()),
                     "lm_score_rows")
    return logprob, rank


def target_stats(llm_handler, formatted_prompt: str, target_text: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per target token, on the CPU: ``(logprob fp32 [T], rank int32 [T])``.  Tokenised as the reference's
    ``_get_logits_and_target_for_scoring`` tokenises - the prompt alone for its length, then the full text, so that merges across the
    boundary are the tokenizer's - and scored in ONE unpadded N = 1 call, so positions are the reference's.  An empty (or wholly
    truncated) target gives empty results without a native call."""
    lm = native_lm(llm_handler)
    if lm is None:
        raise RuntimeError("ace355.lmscore.target_stats: the native LM score is not active on this handler")
    tokenizer = llm_handler.llm_tokenizer
    prompt_len = int(tokenizer(formatted_prompt, return_tensors="pt", add_special_tokens=True)["input_ids"].shape[1])
    full = tokenizer(formatted_prompt + target_text, return_tensors="pt", padding=False, truncation=True, add_special_tokens=True)
    ids = full["input_ids"]
    if ids.shape[1] <= prompt_len:
        return torch.empty(0, dtype=torch.float32), torch.empty(0, dtype=torch.int32)
    mask = full["attention_mask"] if "attention_mask" in full else None
    ctx = getattr(llm_handler, "_load_model_context", None)
    with torch.no_grad(), (ctx() if callable(ctx) else contextlib.nullcontext()):
        logprob, rank = lm.score(ids, mask, start=prompt_len)
        return logprob.cpu(), rank.cpu()


def log_prob_of(logprob: torch.Tensor) -> float:
    """Mean log-probability as the reference takes it (torch fp32 ``.mean().item()``); ``-inf`` for an empty target."""
    if logprob.shape[0] == 0:
        return float("-inf")
    return logprob.to(torch.float32).mean().item()


def topk_recall_of(rank: torch.Tensor, topk: int = 10) -> Tuple[float, Dict[int, float]]:
    """``(position-weighted average, {k: recall at k})`` from 0-based ranks: a hit at k is ``rank < k``; a position weighs
    ``1 - rank / topk`` when ``rank < topk``, else 0."""
    ranks = [int(r) for r in rank.tolist()]
    n = len(ranks)
    if n == 0:
        return 0.0, {}
    recall_per_k = {k: sum(1 for r in ranks if r < k) / n for k in range(1, topk + 1)}
    weights = [1.0 - r / topk if r < topk else 0.0 for r in ranks]
    return sum(weights) / n, recall_per_k


def _native_log_prob(llm_handler, formatted_prompt: str, target_text: str, temperature: float = 1.0) -> float:
    return log_prob_of(target_stats(llm_handler, formatted_prompt, target_text)[0])


def _native_topk_recall(llm_handler, formatted_prompt: str, target_text: str, topk: int = 10) -> Tuple[float, Dict[int, float]]:
    return topk_recall_of(target_stats(llm_handler, formatted_prompt, target_text)[1], topk)


def _think_yaml(fields: Dict[str, Any]) -> str:
    import yaml
    return "<think>\n" + yaml.dump(fields, allow_unicode=True, sort_keys=True).strip() + "\n</think>\n"


def _native_metadata_recall(llm_handler, formatted_prompt: str, fields_dict: Dict[str, Any], topk: int = 10) -> Dict[str, float]:
    out: Dict[str, float] = {}
    for name in sorted(fields_dict or {}):
        out[name], _ = _native_topk_recall(llm_handler, formatted_prompt, _think_yaml({name: fields_dict[name]}), topk=topk)
        logger.debug("Recall for %s: %.4f", name, out[name])
    return out


# ------------------------------------------------------------------------------------------------------------------ score arithmetic
def _own_pmi_to_normalized_score(pmi: float, scale: float = 0.1) -> float:
    """A logistic squash of the PMI: 0.5 at PMI 0, ``scale`` sets the width."""
    return 1.0 / (1.0 + math.exp(-pmi / scale))


def _own_calculate_reward_score(scores: Dict[str, float], weights_config: Optional[Dict[str, float]] = None) -> Tuple[float, str]:
    """Weighted sum of the caption score, the lyrics score and the MEAN of all other (metadata) scores, with weights 0.5 / 0.3 / 0.2
    renormalised over the components present; returns the sum and one breakdown line per component, heaviest first."""
    weights = weights_config if weights_config is not None else {"caption": 0.50, "lyrics": 0.30, "metadata": 0.20}
    meta = [v for k, v in scores.items() if k not in ("caption", "lyrics")]
    present = []
    if scores.get("caption") is not None:
        present.append(("caption", scores["caption"], weights["caption"]))
    if scores.get("lyrics") is not None:
        present.append(("lyrics", scores["lyrics"], weights["lyrics"]))
    if meta:
        present.append(("metadata", sum(meta) / len(meta), weights["metadata"]))
    total_weight = sum(w for _n, _s, w in present)
    if total_weight == 0:
        return 0.0, "❌ No valid scores available to calculate reward."
    total, lines = 0.0, []
    for name, score, w in sorted(present, key=lambda c: c[2], reverse=True):
        share = w / total_weight
        part = score * share
        total += part
        lines.append(f"  • {name.title():<8} | Score: {score:.4f} | Weight: {share:.2f} -> Contrib: +{part:.4f}")
    return total, "\n".join(lines)


def _arith():
    """``(pmi_to_normalized_score, calculate_reward_score)``: the host's when the reference imports, else this package's restatement."""
    ref = _reference()
    if ref is not None:
        return ref.pmi_to_normalized_score, ref.calculate_reward_score
    return _own_pmi_to_normalized_score, _own_calculate_reward_score


def pmi_to_normalized_score(pmi: float, scale: float = 0.1) -> float:
    return _arith()[0](pmi, scale)


def calculate_reward_score(scores: Dict[str, float], weights_config: Optional[Dict[str, float]] = None) -> Tuple[float, str]:
    return _arith()[1](scores, weights_config)


def _native_pmi(llm_handler, audio_codes: str, caption: str, lyrics: str, metadata: Dict[str, Any], topk: int, score_scale: float
                ) -> Tuple[Dict[str, float], float, str]:
    prompt = llm_handler.build_formatted_prompt_for_understanding(audio_codes=audio_codes, is_negative_prompt=False)
    prompt_uncond = llm_handler.build_formatted_prompt_for_understanding(audio_codes="NO USER INPUT", is_negative_prompt=False)
    squash, reward = _arith()

    def pmi(target: str) -> float:
        cond = _native_log_prob(llm_handler, prompt, target)
        uncond = _native_log_prob(llm_handler, prompt_uncond, target)
        return squash(cond - uncond, scale=score_scale)

    scores: Dict[str, float] = {}
    if metadata and isinstance(metadata, dict):
        for key in RECALL_KEYS:
            if metadata.get(key) is not None:
                scores.update(_native_metadata_recall(llm_handler, prompt, {key: metadata[key]}, topk=topk))
        if metadata.get("caption") is not None:
            scores["caption"] = pmi(_think_yaml({"caption": metadata["caption"]}))
    if lyrics:
        scores["lyrics"] = pmi(f"<think>\n</think>\n# Lyric\n{lyrics}\n")
    if not scores:
        return {}, 0.0, "❌ No conditions to evaluate"
    global_score, breakdown = reward(scores)
    lines = [breakdown, "\n✅ Per-condition scores (0-1):"]
    for key, score in sorted(scores.items()):
        lines.append(f"  {key}: {score:.4f} ({'Top-k Recall' if key in RECALL_KEYS else 'PMI (Norm)'})")
    status = "\n".join(lines)
    logger.info("Calculated scores: %.4f\n%s", global_score, status)
    return scores, global_score, status


# ------------------------------------------------------------------------------------------------------------------ the entry points
def calculate_log_prob(llm_handler, formatted_prompt: str, target_text: str, temperature: float = 1.0) -> float:
    """Mean log-probability of ``target_text`` after ``formatted_prompt`` (``temperature`` is accepted and ignored, as in the reference)."""
    return _routed("_calculate_log_prob", _native_log_prob, llm_handler, formatted_prompt, target_text, temperature)


def calculate_topk_recall(llm_handler, formatted_prompt: str, target_text: str, topk: int = 10) -> Tuple[float, Dict[int, float]]:
    return _routed("_calculate_topk_recall", _native_topk_recall, llm_handler, formatted_prompt, target_text, topk=topk)


def calculate_metadata_recall(llm_handler, formatted_prompt: str, fields_dict: Dict[str, Any], topk: int = 10) -> Dict[str, float]:
    return _routed("_calculate_metadata_recall", _native_metadata_recall, llm_handler, formatted_prompt, fields_dict, topk=topk)


def calculate_pmi_score_per_condition(llm_handler, audio_codes: str, caption: str = "", lyrics: str = "",
                                      metadata: Optional[Dict[str, Any]] = None, temperature: float = 1.0, topk: int = 10,
                                      score_scale: float = 0.1) -> Tuple[Dict[str, float], float, str]:
    """``(scores per condition, global score, status text)``: top-k recall for the metadata fields, normalised PMI for caption and lyrics."""
    err: Optional[BaseException] = None
    if native_lm(llm_handler) is not None:
        if not llm_handler.llm_initialized:
            return {}, 0.0, "❌ LLM not initialized"
        if not audio_codes or not audio_codes.strip():
            return {}, 0.0, "❌ No audio codes provided"
        if "caption" not in metadata:
            metadata["caption"] = caption
        try:
            return _native_pmi(llm_handler, audio_codes, caption, lyrics, metadata, topk, score_scale)
        except Exception as exc:
            _note_failure(exc)
            err = exc
    ref = _reference()
    if ref is None:
        if err is None:
            err = RuntimeError("the native LM score is not active and acestep.core.scoring.lm_score does not import")
        error_msg = f"❌ Error: {str(err)}"
        logger.error(error_msg)
        return {}, float("-inf"), error_msg
    return ref.calculate_pmi_score_per_condition(llm_handler, audio_codes, caption=caption, lyrics=lyrics, metadata=metadata,
                                                 temperature=temperature, topk=topk, score_scale=score_scale)
