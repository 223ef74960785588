"""The logits stage of the 5 Hz LM's CFG loop, and the loop itself with a codes phase that never leaves the GPU.

Between its forward and its token selection the reference's ``_generate_with_cfg_custom`` (llm_inference.py:2414-2533) runs, per token:
the CFG combine (``:2482``), ``MetadataConstrainedLogitsProcessor.__call__`` (constrained_logits_processor.py:1568-1639) and
transformers' ``RepetitionPenaltyLogitsProcessor``; then ``_update_constrained_processor_state`` reads every token with ``.item()``,
``_check_eos_token`` reads two ``torch.any`` and the ids grow by a ``torch.cat``.  Here:

* ``shape_logits`` is the stage as one native launch (``ace355_lm_shape``; semantics, exactly: include/ace355.h above that call);
* ``SeenTokens`` is the bitmap of ids the repetition penalty reads (``ace355_lm_seen_mark``);
* ``step_plan`` decides, from the processor's attributes alone, what one step of the loop is;
* ``generate_with_cfg`` is the loop (``NativeLmMixin._generate_with_cfg_custom`` calls it when ``use_native_lm_loop`` is set);
* ``generate_codes_batch`` is that loop for B songs that share one prompt, each with the tokens the loop gives it alone, and
  ``batch_request`` decides which ``_run_pt`` calls are such batches (``NativeLmMixin._run_pt``, ``use_native_lm_batch``);
* ``_cfg_loop`` is the one loop behind both: each of the two builds a ``_LoopMode`` and formats what the loop returns;
* ``generate_constrained`` and ``generate_codes_batch_nocfg`` are that loop without CFG (``_LoopMode.cfg`` False: the reference's
  ``_generate_with_constrained_decoding``, stage in the model's dtype), ``nocfg_batch_request`` is ``batch_request`` for them
  (``NativeLmMixin._generate_with_constrained_decoding`` / ``_run_pt``, ``use_native_lm_nocfg``).

The native stage covers the processor's branches that are a fixed mask plus one EOS rule: no processor, a disabled one, ``COMPLETED``
and ``CODES_GENERATION``.  Every other FSM state runs the reference's own torch code on the native forward's logits, as before.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple, Optional

import torch

from . import native

NEG_INF = float("-inf")
MIN_TEMPERATURE = 1e-6   # _apply_temperature_scaling's stand-in for T <= 0 (constrained_logits_processor.py:1691-1692)


# ---------------------------------------------------------------------------------------------------------------- the stage
def _rows(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        raise ValueError(f"ace355: {what} must be fp32 [B, V] on the GPU with unit column stride (rows may be strided)")
    return x


class SeenTokens:
    """Which ids each of B rows has seen: ``words`` is int32 ``[B, ceil(V / 32)]`` on the GPU, bit ``v & 31`` of word ``v >> 5``."""

    def __init__(self, B: int, V: int, device):
        if not 1 <= B <= native.LM_MAX_SEQS or not 1 <= V <= native.LM_PICK_MAX_V:
            raise ValueError(f"ace355: SeenTokens takes 1 .. {native.LM_MAX_SEQS} rows of 1 .. {native.LM_PICK_MAX_V} ids")
        self.B, self.V = int(B), int(V)
        self.words = torch.zeros(self.B, (self.V + 31) // 32, dtype=torch.int32, device=device)

    def mark(self, ids: torch.Tensor) -> "SeenTokens":
        """``ids`` int64 ``[B, T]`` (or ``[B]``) on the GPU, rows may be strided: every id in [0, V) sets its bit, others are ignored."""
        if ids.dim() == 1:
            ids = ids[:, None]
        if ids.dim() != 2 or ids.shape[0] != self.B or ids.dtype != torch.int64 or ids.device != self.words.device:
            raise ValueError(f"ace355: SeenTokens.mark takes int64 ids [{self.B}, T] on {self.words.device}")
        T = ids.shape[1]
        if T == 0:
            return self
        if ids.stride(1) != 1 or ids.stride(0) < T:
            ids = ids.contiguous()
        with torch.cuda.device(ids.device):
            for t0 in range(0, T, native.LM_MAX_POSITIONS):
                part = ids[:, t0:t0 + native.LM_MAX_POSITIONS]
                native.check(native.lib().ace355_lm_seen_mark(part.data_ptr(), ids.stride(0), self.B, part.shape[1], self.V,
                                                              self.words.data_ptr(), native.current_stream_ptr()), "lm_seen_mark")
        return self


def shape_logits(cond: torch.Tensor, uncond: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, mask: Optional[torch.Tensor] = None,
                 eos_id: Optional[int] = None, eos_mode: int = native.LM_EOS_NONE, temperature: Optional[float] = None,
                 penalty: float = 1.0, seen: Optional[SeenTokens] = None, out: Optional[torch.Tensor] = None,
                 dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The logits stage on ``cond`` / ``uncond`` (fp32 ``[B, V]`` on the GPU, rows may be strided, B <= 16; ``uncond=None``: no CFG):
    CFG combine, ``+ mask``, the EOS rule, ``/ temperature`` (``None``: skipped; ``<= 0``: 1e-6, as the reference), repetition penalty
    on the ids ``seen`` holds.  One launch on the current stream.  Returns ``out`` (default: a new ``[B, V]``; may be ``cond``).
    ``dtype`` None or ``torch.float32``: every operation rounds to fp32 (``ace355_lm_shape``).  ``torch.bfloat16``: the logits and every
    result round to bf16, as torch rounds them on a bf16 tensor (``ace355_lm_shape_as``; no ``uncond``); ``out`` is fp32 all the same."""
    if dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError(f"ace355: the logits stage runs in torch.float32 or torch.bfloat16, not {dtype}")
    if dtype == torch.bfloat16 and uncond is not None:
        raise ValueError("ace355: the bf16 logits stage takes no uncond (the reference combines in fp32)")
    cond = _rows(cond, "cond")
    B, V = cond.shape
    if uncond is not None and _rows(uncond, "uncond").shape != (B, V):
        raise ValueError("ace355: uncond must have cond's shape")
    if out is None:
        out = torch.empty(B, V, dtype=torch.float32, device=cond.device)
    elif _rows(out, "out").shape != (B, V) or out.device != cond.device:
        raise ValueError("ace355: out must have cond's shape and device")
    if mask is not None and (mask.dtype != torch.float32 or mask.device != cond.device or mask.shape != (V,) or not mask.is_contiguous()):
        raise ValueError("ace355: mask must be a contiguous fp32 [V] on the logits' device")
    penalty = float(penalty)
    if penalty != 1.0 and (seen is None or seen.B != B or seen.V != V or seen.words.device != cond.device):
        raise ValueError("ace355: a repetition penalty needs SeenTokens of the logits' shape and device")
    T = None if temperature is None else (float(temperature) if temperature > 0 else MIN_TEMPERATURE)
    p = native.LmShapeParamsC(cfg_scale=float(cfg_scale), eos_id=int(eos_id) if eos_id is not None else -1, eos_mode=int(eos_mode),
                              has_temperature=0 if T is None else 1, temperature=T or 0.0, penalty=penalty,
                              mask=mask.data_ptr() if mask is not None else None,
                              seen=seen.words.data_ptr() if penalty != 1.0 else None)
    with torch.cuda.device(cond.device):
        if dtype == torch.bfloat16:
            native.check(native.lib().ace355_lm_shape_as(cond.data_ptr(), cond.stride(0), None, 0, out.data_ptr(), out.stride(0), B, V,
                                                         C.byref(p), native.DTYPE_BF16, native.current_stream_ptr()), "lm_shape_as")
            return out
        native.check(native.lib().ace355_lm_shape(cond.data_ptr(), cond.stride(0), uncond.data_ptr() if uncond is not None else None,
                                                  uncond.stride(0) if uncond is not None else 0, out.data_ptr(), out.stride(0), B, V,
                                                  C.byref(p), native.current_stream_ptr()), "lm_shape")
    return out


# ---------------------------------------------------------------------------------------------------------------- what a step is
class StepView(NamedTuple):
    """What ``step_plan`` may look at.  ``processor``: the ``MetadataConstrainedLogitsProcessor`` or None.  ``eos_token_id`` /
    ``pad_token_id``: the ids ``_check_eos_token`` stops the loop on (pad may be None).  ``blocked``: ids known to be ``-inf`` in the
    processor's ``non_audio_code_mask`` (the loop reads them once per call); None: ``step_plan`` reads the mask itself."""
    processor: Any
    eos_token_id: int
    pad_token_id: Optional[int]
    has_streamer: bool
    blocked: Optional[frozenset] = None


class StepPlan(NamedTuple):
    native: bool                    # the stage is ace355_lm_shape; False: the reference's processor runs
    mask: Optional[torch.Tensor]    # added to the logits, or None
    eos_mode: int                   # native.LM_EOS_NONE / LM_EOS_BLOCK / LM_EOS_FORCE, on processor.eos_token_id
    temperature: Optional[float]    # the processor's temperature for this state, or None
    sync_free: bool                 # no token this step can draw stops the loop or steers the processor: nothing is read back


def _state_name(state) -> str:
    return getattr(state, "name", state)


def step_plan(view: StepView) -> StepPlan:
    """Pure: reads ``view`` and the processor's attributes (``enabled``, ``state``, ``generation_phase``, ``audio_code_mask``,
    ``non_audio_code_mask``, ``target_codes``, ``codes_count``, ``eos_token_id``, ``metadata_temperature``, ``codes_temperature``) and
    changes nothing.  The branches are those of ``MetadataConstrainedLogitsProcessor.__call__`` (constrained_logits_processor.py:
    1583-1629) that end in ``_apply_temperature_scaling`` without an FSM walk."""
    p = view.processor
    if p is None:
        return StepPlan(True, None, native.LM_EOS_NONE, None, False)
    state = _state_name(p.state)
    T = p.codes_temperature if state in ("CODES_GENERATION", "COMPLETED") else p.metadata_temperature
    if not p.enabled:
        return StepPlan(True, None, native.LM_EOS_NONE, T, False)
    if state == "COMPLETED":
        mask = p.audio_code_mask if p.generation_phase == "understand" else None
        return StepPlan(True, mask, native.LM_EOS_NONE, T, False)
    if state != "CODES_GENERATION":
        return StepPlan(False, None, native.LM_EOS_NONE, None, False)   # (THINK_TAG of a codes-phase call included: __call__ makes the jump)
    mask = p.non_audio_code_mask
    mode = native.LM_EOS_NONE
    if p.target_codes is not None and p.eos_token_id is not None:
        mode = native.LM_EOS_BLOCK if p.codes_count < p.target_codes else native.LM_EOS_FORCE
    sync_free = mode == native.LM_EOS_BLOCK and mask is not None and not view.has_streamer
    if sync_free:   # every id the loop stops on is either the blocked EOS or -inf in the mask
        stops = {view.eos_token_id} | ({view.pad_token_id} if view.pad_token_id is not None else set())
        for t in stops - {p.eos_token_id}:
            if view.blocked is not None:
                ok = t in view.blocked
            else:
                ok = 0 <= t < mask.shape[-1] and float(mask.reshape(-1)[t]) == NEG_INF
            sync_free = sync_free and ok
    return StepPlan(True, mask, mode, T, sync_free)


# ---------------------------------------------------------------------------------------------------------------- the loop
def _codes_mask(processor, name: str, device) -> Optional[torch.Tensor]:
    """The processor's mask as the stage takes it.  Like the reference's ``__call__`` (``:1589-1591``, ``:1611-1612``) this moves the
    processor's own attribute to the logits' device and dtype (fp32: the CFG result is, and the non-CFG stage takes its mask in
    fp32 and rounds it itself; 0 and -inf are exact in every dtype)."""
    m = getattr(processor, name)
    if m is None:
        return None
    if m.device != device or m.dtype != torch.float32:
        m = m.to(device=device, dtype=torch.float32)
        setattr(processor, name, m)
    return m if m.dim() == 1 and m.is_contiguous() else m.reshape(-1).contiguous()


class _LoopMode(NamedTuple):
    """Which loop ``_cfg_loop`` runs.  ``seeds`` None: ``generate_with_cfg``, the rows of the ids are B conditional + B unconditional
    prompts and the global generator draws.  ``seeds`` a list: ``generate_codes_batch``, the ids are one ``[2, P]`` pair for
    ``B = len(seeds)`` songs, row i draws from a generator of its own seeded ``seeds[i]``, and there is no streamer.  ``cfg`` False:
    the non-CFG loop (``generate_constrained`` / ``generate_codes_batch_nocfg``): the ids hold no unconditional rows (B prompts, or
    one ``[1, P]`` prompt for the songs of ``seeds``), and the stage runs in the model's dtype on the forward's fp32 logits, as the
    reference's ``_generate_with_constrained_decoding`` does (llm_inference.py:2369-2377: no upcast)."""
    B: int                  # token rows
    seeds: Optional[list]
    streamer: Any
    cfg: bool = True


def _cfg_loop(handler, lm, ids: torch.Tensor, attention_mask: Optional[torch.Tensor], mode: _LoopMode, max_new_tokens: int,
              temperature: float, cfg_scale: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float,
              pad_token_id: int, proc) -> torch.Tensor:
    """The loop behind ``generate_with_cfg``, ``generate_codes_batch`` and their non-CFG counterparts (``cfg_scale`` is not read
    there): int64 ``[steps, B]``, row t the tokens of step t.  Leaves ``handler._lm_loop_stats``; raises when some step could draw
    no token."""
    from . import lmsample
    B, streamer, batched, cfg = mode.B, mode.streamer, mode.seeds is not None, mode.cfg
    dev = ids.device
    n0 = 1 if batched else B   # conditional rows of the prompt, and of step 0's logits
    V = lm.cfg.vocab_size
    eos = handler.llm_tokenizer.eos_token_id
    if eos is None:
        eos = pad_token_id
    penalty = float(repetition_penalty)
    sample = temperature > 0
    stats = {"steps": 0, "native_steps": 0, "sync_free_steps": 0, "token_reads": 0}
    if batched:
        stats.update(batch=B, prefill_rows=2 if cfg else 1)
    if not cfg:
        stats["cfg"] = False
    handler._lm_loop_stats = stats
    tokens = torch.empty(max(int(max_new_tokens), 1), B, dtype=torch.int64, device=dev)   # row t: the tokens of step t
    # the conditional rows, pads included; batched: every song's is the pair's
    seen = SeenTokens(B, V, dev).mark(ids[:n0].to(torch.int64).expand(B, ids.shape[1])) if penalty != 1.0 else None
    gens = [torch.Generator(device=dev).manual_seed(s) for s in mode.seeds] if batched and sample else []
    u = torch.empty(B, dtype=torch.float32, device=dev) if gens else None
    stop_ids = {eos} | ({pad_token_id} if pad_token_id is not None else set())
    blocked, blocked_for = None, None
    steps, bad_draw = 0, False
    lm.bad_tokens()   # whatever an earlier user of the handle left uncounted is not this call's

    with torch.inference_mode():
        for step in range(int(max_new_tokens)):
            logits = lm.prefill(ids, attention_mask) if step == 0 else lm.decode_tokens(tokens[step - 1])
            if cfg and lm.out_dtype != torch.float32:
                logits = logits.to(lm.out_dtype).float()   # the model's own output dtype, upcast as llm_inference.py:2482 does
            n = n0 if step == 0 else B
            cond, uncond = (logits[:n], logits[n:]) if cfg else (logits, None)   # no CFG: the stage's first rounding is the .to(dtype)
            if proc is not None and proc.enabled and _state_name(proc.state) == "CODES_GENERATION" and proc.non_audio_code_mask is not None:
                m = _codes_mask(proc, "non_audio_code_mask", dev)
                if blocked_for is not proc.non_audio_code_mask:   # once per call: which of the loop's stop ids the mask rules out
                    known = [t for t in stop_ids if 0 <= t < m.shape[0]]
                    vals = m[torch.tensor(known, dtype=torch.int64, device=dev)].tolist() if known else []
                    blocked = frozenset(t for t, v in zip(known, vals) if v == NEG_INF)
                    blocked_for = proc.non_audio_code_mask
            plan = step_plan(StepView(proc, eos, pad_token_id, streamer is not None, blocked))
            if plan.native:
                if n != B:   # one staged row per song: the penalty's bitmap and the selection have B rows
                    cond, uncond = cond.repeat(B, 1), uncond.repeat(B, 1) if cfg else None
                mask = None
                if plan.mask is not None:
                    mask = _codes_mask(proc, "audio_code_mask" if _state_name(proc.state) == "COMPLETED" else "non_audio_code_mask", dev)
                if cfg:
                    x = shape_logits(cond, uncond, cfg_scale, mask, proc.eos_token_id if plan.eos_mode else None, plan.eos_mode,
                                     plan.temperature, penalty, seen, out=cond)
                else:
                    x = shape_logits(cond, None, 1.0, mask, proc.eos_token_id if plan.eos_mode else None, plan.eos_mode,
                                     plan.temperature, penalty, seen, out=cond, dtype=lm.out_dtype)
                stats["native_steps"] += 1
            else:   # the reference's processor (THINK_TAG -> CODES_GENERATION is made in its __call__)
                if batched and step != 0:
                    raise RuntimeError(f"ace355: the constrained processor left the codes phase at step {step} of a batched loop "
                                       f"(state {_state_name(proc.state)})")
                cur = ids[:1] if batched else torch.cat([ids[:B], tokens[:step].t().to(ids.dtype)], dim=1)
                x = uncond + cfg_scale * (cond - uncond) if cfg else cond.to(lm.out_dtype)
                x = proc(cur, x)
                for lp in handler._build_logits_processor(repetition_penalty):
                    x = lp(cur, x)
                if not cfg:
                    x = x.float()   # the selection reads fp32; the values stay the model dtype's
                if batched:
                    x = x.repeat(B, 1)
            if batched:   # row i's own stream of uniforms: one torch.rand(1) per step, as the B = 1 loop draws
                for i, g in enumerate(gens):
                    torch.rand(1, generator=g, out=u[i:i + 1])
            elif plan.native and sample:
                u = torch.rand(B, device=dev)
            if plan.native or batched:
                toks = lmsample.pick(x, top_k, top_p, temperature, u)[0]
            else:
                toks = lmsample.select_tokens(x, top_k, top_p, temperature, check=False)
            tokens[step] = toks
            steps = step + 1
            if seen is not None:
                seen.mark(tokens[step])
            if batched and step == 0:
                lm.fan_out([0] * B + [1] * B if cfg else [0] * B)
            if plan.native and plan.sync_free:
                for _ in range(1 if batched else B):   # batched: once per step, codes per song
                    proc.update_state(0)   # CODES_GENERATION only counts (update_state :2153-2158): the value is not looked at
                stats["sync_free_steps"] += 1
                continue
            host = toks.tolist()
            stats["token_reads"] += 1
            if min(host) < 0:
                bad_draw = True
                break
            if batched:
                proc.update_state(host[0])
                if _state_name(proc.state) != "CODES_GENERATION":
                    raise RuntimeError(f"ace355: the constrained processor is in state {_state_name(proc.state)} after step {step} of a "
                                       f"batched loop; only the codes phase runs batched")
            elif proc is not None:
                for t in host:
                    proc.update_state(t)
            if streamer is not None:
                streamer.put(toks.unsqueeze(1))
            stopped = [t in stop_ids for t in host]
            if batched and any(stopped) and not all(stopped):
                raise RuntimeError(f"ace355: songs {[i for i, s in enumerate(stopped) if s]} of {B} stopped at step {step} and the "
                                   f"others did not; the batched LM loop returns no ragged rows")
            if any(stopped):
                break
    stats["steps"] = steps
    if streamer is not None:
        streamer.end()
    replaced = lm.bad_tokens() if steps > 1 else 0
    if not bad_draw and steps:
        bad_draw = bool((tokens[:steps] < 0).any())
    if bad_draw or replaced:
        raise RuntimeError(f"ace355: the native LM loop drew no valid token at some step (a logits row with a NaN, a +inf or no finite "
                           f"entry; {replaced} ids replaced in the forward); the constrained processor has advanced {steps} steps")
    return tokens[:steps]


def generate_with_cfg(handler, lm, batch_input_ids: torch.Tensor, batch_attention_mask: Optional[torch.Tensor], max_new_tokens: int,
                      temperature: float, cfg_scale: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float,
                      pad_token_id: int, streamer, constrained_processor=None) -> torch.Tensor:
    """``LLMHandler._generate_with_cfg_custom`` on ``lm`` (a ``NativeCausalLM``): same arguments, same return (``[2B, P + steps]``,
    conditional rows first), same streamer calls, the processor left as the reference's loop leaves it.  The draw is the native
    selection's (``lmsample``: one ``torch.rand(B)`` per step), not ``torch.multinomial``'s.  ``handler`` supplies ``llm_tokenizer`` and
    ``_build_logits_processor`` (the latter only on a reference step).  Leaves ``handler._lm_loop_stats``."""
    ids = batch_input_ids
    tokens = _cfg_loop(handler, lm, ids, batch_attention_mask, _LoopMode(ids.shape[0] // 2, None, streamer), max_new_tokens, temperature,
                       cfg_scale, top_k, top_p, repetition_penalty, pad_token_id, constrained_processor)
    return torch.cat([ids, tokens.t().repeat(2, 1).to(ids.dtype)], dim=1)


# ---------------------------------------------------------------------------------------------------------------- B songs, one loop
def batch_request(formatted_prompts, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds,
                  loop_refusal: Optional[str] = None):
    """``(ok, why)``: may a ``_run_pt`` call run as one batched loop (``generate_codes_batch``)?  Pure.  The reference's only batch
    caller passes the same prompt B times with B seeds (llm_inference.py:1314-1373); everything else stays sequential.
    ``loop_refusal``: why ``NativeLmMixin._lm_loop_accepts`` turned the tokenised pair down, once that is known."""
    if not isinstance(formatted_prompts, list) or len(formatted_prompts) < 2:
        return False, "the prompts are not a list of two or more"
    if any(not isinstance(p, str) or p != formatted_prompts[0] for p in formatted_prompts):
        return False, "the prompts of the batch differ"
    if not cfg_scale > 1.0:
        return False, f"cfg_scale {cfg_scale} runs no CFG pair"
    if generation_phase != "codes":
        return False, f"generation phase '{generation_phase}' is not 'codes'"
    if not use_constrained_decoding:
        return False, "constrained decoding is off, so nothing ends every song at the same step"
    if target_duration is None or not target_duration > 0:
        return False, "no target duration, so nothing ends every song at the same step"
    if (not isinstance(seeds, (list, tuple)) or len(seeds) < len(formatted_prompts)
            or any(isinstance(s, bool) or not isinstance(s, int) for s in seeds[:len(formatted_prompts)])):
        return False, "seeds does not hold an int for every item"
    if loop_refusal is not None:
        return False, loop_refusal
    return True, None


def generate_codes_batch(handler, lm, pair_ids: torch.Tensor, pair_mask: Optional[torch.Tensor], seeds, max_new_tokens: int,
                         temperature: float, cfg_scale: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float,
                         pad_token_id: int, constrained_processor) -> torch.Tensor:
    """The audio codes of ``B = len(seeds)`` songs that share one prompt, in one CFG loop: int64 ``[B, P + steps]``, the B conditional
    rows.  Row i equals the conditional row of ``generate_with_cfg(handler, lm, pair_ids, pair_mask, ...)`` called right after
    ``torch.manual_seed(seeds[i]); torch.cuda.manual_seed_all(seeds[i])`` with a freshly reset processor - what the reference's
    ``_run_pt`` does per item (llm_inference.py:1021-1059).

    ``pair_ids`` ``[2, P]``: the conditional and the unconditional prompt, left-padded.  The pair is prefilled once; its staged row
    is expanded to B rows, B tokens are selected, the cache is fanned out to B conditional + B unconditional sequences
    (``lm.fan_out``) and every later step decodes all 2B.  Row i draws its uniforms from a generator of its own, seeded ``seeds[i]``:
    the t-th is the t-th ``torch.rand(1)`` after that seeding, and the global generators are not touched.  The processor counts once
    per step (codes per song) and is left as the last sequential item would leave it.  Needs an enabled processor with
    ``target_codes`` and ``eos_token_id``: EOS is blocked until the count is reached and then forced, so every row stops at the same
    step; a step that finds only some rows stopped raises.  Leaves ``handler._lm_loop_stats`` (plus ``batch``, ``prefill_rows``)."""
    proc = constrained_processor
    if proc is None or not proc.enabled or proc.target_codes is None or proc.eos_token_id is None:
        raise RuntimeError("ace355: the batched LM loop needs an enabled constrained processor with target_codes and eos_token_id "
                           "(nothing else ends every song at the same step)")
    seeds = [int(s) for s in seeds]
    B = len(seeds)
    if pair_ids.dim() != 2 or pair_ids.shape[0] != 2:
        raise ValueError("ace355: the batched LM loop takes the [2, P] pair of conditional and unconditional ids")
    if not 1 <= B or 2 * B > lm.max_seqs:
        raise ValueError(f"ace355: {B} songs need {2 * B} sequences, the native LM holds {lm.max_seqs}")
    tokens = _cfg_loop(handler, lm, pair_ids, pair_mask, _LoopMode(B, seeds, None), max_new_tokens, temperature, cfg_scale, top_k, top_p,
                       repetition_penalty, pad_token_id, proc)
    return torch.cat([pair_ids[:1].to(torch.int64).expand(B, pair_ids.shape[1]), tokens.t()], dim=1)


# ---------------------------------------------------------------------------------------------------------------- without CFG
def _nocfg_dtype(lm):
    if lm.out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"ace355: the native non-CFG LM loop runs its stage in fp32 or bf16, the LM's out_dtype is {lm.out_dtype}")


def generate_constrained(handler, lm, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], max_new_tokens: int,
                         temperature: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float, pad_token_id: int,
                         streamer, constrained_processor=None) -> torch.Tensor:
    """``LLMHandler._generate_with_constrained_decoding`` (llm_inference.py:2321-2412) on ``lm`` (a ``NativeCausalLM``): same
    arguments, same return (``[B, P + steps]``), same streamer calls, the processor left as the reference's loop leaves it.  The
    third mode of ``_cfg_loop``: B sequences and no unconditional rows, the stage in ``lm.out_dtype`` (that loop never upcasts, so a
    bf16 model's processor results round to bf16; ``shape_logits(dtype=...)``), and on an FSM state ``step_plan`` does not cover the
    reference's processor on ``logits.to(lm.out_dtype)``.  The loop ends after the step in which any row drew the tokenizer's EOS or
    ``pad_token_id`` (``_check_eos_token``).  The draw is the native selection's, as in ``generate_with_cfg``.  Leaves
    ``handler._lm_loop_stats`` (plus ``"cfg": False``)."""
    _nocfg_dtype(lm)
    ids = input_ids
    tokens = _cfg_loop(handler, lm, ids, attention_mask, _LoopMode(ids.shape[0], None, streamer, False), max_new_tokens, temperature, 1.0,
                       top_k, top_p, repetition_penalty, pad_token_id, constrained_processor)
    return torch.cat([ids, tokens.t().to(ids.dtype)], dim=1)


def nocfg_batch_request(formatted_prompts, cfg_scale, generation_phase, use_constrained_decoding, target_duration, seeds,
                        loop_refusal: Optional[str] = None):
    """``batch_request`` for the non-CFG loop (``generate_codes_batch_nocfg``): the same conditions with the CFG one reversed - the
    reference takes this branch when ``not cfg_scale > 1.0`` (llm_inference.py:929).  Pure."""
    if not isinstance(formatted_prompts, list) or len(formatted_prompts) < 2:
        return False, "the prompts are not a list of two or more"
    if any(not isinstance(p, str) or p != formatted_prompts[0] for p in formatted_prompts):
        return False, "the prompts of the batch differ"
    if cfg_scale > 1.0:
        return False, f"cfg_scale {cfg_scale} runs a CFG pair"
    if generation_phase != "codes":
        return False, f"generation phase '{generation_phase}' is not 'codes'"
    if not use_constrained_decoding:
        return False, "constrained decoding is off, so nothing ends every song at the same step"
    if target_duration is None or not target_duration > 0:
        return False, "no target duration, so nothing ends every song at the same step"
    if (not isinstance(seeds, (list, tuple)) or len(seeds) < len(formatted_prompts)
            or any(isinstance(s, bool) or not isinstance(s, int) for s in seeds[:len(formatted_prompts)])):
        return False, "seeds does not hold an int for every item"
    if loop_refusal is not None:
        return False, loop_refusal
    return True, None


def generate_codes_batch_nocfg(handler, lm, prompt_ids: torch.Tensor, prompt_mask: Optional[torch.Tensor], seeds, max_new_tokens: int,
                               temperature: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float,
                               pad_token_id: int, constrained_processor) -> torch.Tensor:
    """``generate_codes_batch`` without CFG: the audio codes of ``B = len(seeds)`` songs that share the ``[1, P]`` prompt, int64
    ``[B, P + steps]``.  One prefill of the prompt; its staged row is expanded to B rows, B tokens are selected, the cache is fanned
    out to B sequences (``lm.fan_out([0] * B)``) and every later step decodes all B - up to ``lm.max_seqs`` songs, twice the CFG
    path's.  Row i equals ``generate_constrained`` on the prompt called right after ``torch.manual_seed(seeds[i]);
    torch.cuda.manual_seed_all(seeds[i])`` with a fresh processor; its uniforms come from a generator of its own, and the global
    generators are not touched.  Needs an enabled processor with ``target_codes`` and ``eos_token_id``; a step that finds only some
    rows stopped raises.  Leaves ``handler._lm_loop_stats`` (plus ``batch``, ``prefill_rows`` 1, ``"cfg": False``)."""
    proc = constrained_processor
    if proc is None or not proc.enabled or proc.target_codes is None or proc.eos_token_id is None:
        raise RuntimeError("ace355: the batched LM loop needs an enabled constrained processor with target_codes and eos_token_id "
                           "(nothing else ends every song at the same step)")
    _nocfg_dtype(lm)
    seeds = [int(s) for s in seeds]
    B = len(seeds)
    if prompt_ids.dim() != 2 or prompt_ids.shape[0] != 1:
        raise ValueError("ace355: the batched non-CFG LM loop takes the [1, P] ids of the one prompt")
    if not 1 <= B <= lm.max_seqs:
        raise ValueError(f"ace355: {B} songs need {B} sequences, the native LM holds {lm.max_seqs}")
    tokens = _cfg_loop(handler, lm, prompt_ids, prompt_mask, _LoopMode(B, seeds, None, False), max_new_tokens, temperature, 1.0, top_k,
                       top_p, repetition_penalty, pad_token_id, proc)
    return torch.cat([prompt_ids.to(torch.int64).expand(B, prompt_ids.shape[1]), tokens.t()], dim=1)
