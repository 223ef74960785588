"""The logits stage of the 5 Hz LM's CFG loop, and the loop itself with a codes phase that never leaves the GPU.

Between its forward and its token selection the reference's ``_generate_with_cfg_custom`` (llm_inference.py:2414-2533) runs, per token:
the CFG combine (``:2482``), ``MetadataConstrainedLogitsProcessor.__call__`` (constrained_logits_processor.py:1568-1639) and
transformers' ``RepetitionPenaltyLogitsProcessor``; then ``_update_constrained_processor_state`` reads every token with ``.item()``,
``_check_eos_token`` reads two ``torch.any`` and the ids grow by a ``torch.cat``.  Here:

* ``shape_logits`` is the stage as one native launch (``ace355_lm_shape``; semantics, exactly: include/ace355.h above that call);
* ``SeenTokens`` is the bitmap of ids the repetition penalty reads (``ace355_lm_seen_mark``);
* ``step_plan`` decides, from the processor's attributes alone, what one step of the loop is;
* ``generate_with_cfg`` is the loop (``NativeLmMixin._generate_with_cfg_custom`` calls it when ``use_native_lm_loop`` is set).

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
                 penalty: float = 1.0, seen: Optional[SeenTokens] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The logits stage on ``cond`` / ``uncond`` (fp32 ``[B, V]`` on the GPU, rows may be strided, B <= 16; ``uncond=None``: no CFG):
    CFG combine, ``+ mask``, the EOS rule, ``/ temperature`` (``None``: skipped; ``<= 0``: 1e-6, as the reference), repetition penalty
    on the ids ``seen`` holds.  One launch on the current stream.  Returns ``out`` (default: a new ``[B, V]``; may be ``cond``)."""
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
    processor's own attribute to the logits' device and dtype (fp32: the CFG result is)."""
    m = getattr(processor, name)
    if m is None:
        return None
    if m.device != device or m.dtype != torch.float32:
        m = m.to(device=device, dtype=torch.float32)
        setattr(processor, name, m)
    return m if m.dim() == 1 and m.is_contiguous() else m.reshape(-1).contiguous()


def generate_with_cfg(handler, lm, batch_input_ids: torch.Tensor, batch_attention_mask: Optional[torch.Tensor], max_new_tokens: int,
                      temperature: float, cfg_scale: float, top_k: Optional[int], top_p: Optional[float], repetition_penalty: float,
                      pad_token_id: int, streamer, constrained_processor=None) -> torch.Tensor:
    """``LLMHandler._generate_with_cfg_custom`` on ``lm`` (a ``NativeCausalLM``): same arguments, same return (``[2B, P + steps]``,
    conditional rows first), same streamer calls, the processor left as the reference's loop leaves it.  The draw is the native
    selection's (``lmsample``: one ``torch.rand(B)`` per step), not ``torch.multinomial``'s.  ``handler`` supplies ``llm_tokenizer`` and
    ``_build_logits_processor`` (the latter only on a reference step).  Leaves ``handler._lm_loop_stats``."""
    from . import lmsample
    ids = batch_input_ids
    dev = ids.device
    B = ids.shape[0] // 2
    V = lm.cfg.vocab_size
    eos = handler.llm_tokenizer.eos_token_id
    if eos is None:
        eos = pad_token_id
    proc = constrained_processor
    penalty = float(repetition_penalty)
    sample = temperature > 0
    stats = {"steps": 0, "native_steps": 0, "sync_free_steps": 0, "token_reads": 0}
    handler._lm_loop_stats = stats
    tokens = torch.empty(max(int(max_new_tokens), 1), B, dtype=torch.int64, device=dev)   # row t: the tokens of step t
    seen = SeenTokens(B, V, dev).mark(ids[:B].to(torch.int64)) if penalty != 1.0 else None   # the conditional rows, pads included
    blocked, blocked_for = None, None
    steps, bad_draw = 0, False
    lm.bad_tokens()   # whatever an earlier user of the handle left uncounted is not this call's

    with torch.inference_mode():
        for step in range(int(max_new_tokens)):
            logits = lm.prefill(ids, batch_attention_mask) if step == 0 else lm.decode_tokens(tokens[step - 1])
            if lm.out_dtype != torch.float32:
                logits = logits.to(lm.out_dtype).float()   # the model's own output dtype, upcast as llm_inference.py:2482 does
            cond, uncond = logits[:B], logits[B:]
            if proc is not None and proc.enabled and _state_name(proc.state) == "CODES_GENERATION" and proc.non_audio_code_mask is not None:
                m = _codes_mask(proc, "non_audio_code_mask", dev)
                if blocked_for is not proc.non_audio_code_mask:   # once per call: which of the loop's stop ids the mask rules out
                    stop_ids = [t for t in {eos, pad_token_id} if t is not None and 0 <= t < m.shape[0]]
                    vals = m[torch.tensor(stop_ids, dtype=torch.int64, device=dev)].tolist() if stop_ids else []
                    blocked = frozenset(t for t, v in zip(stop_ids, vals) if v == NEG_INF)
                    blocked_for = proc.non_audio_code_mask
            plan = step_plan(StepView(proc, eos, pad_token_id, streamer is not None, blocked))
            if plan.native:
                mask = None
                if plan.mask is not None:
                    mask = _codes_mask(proc, "audio_code_mask" if _state_name(proc.state) == "COMPLETED" else "non_audio_code_mask", dev)
                x = shape_logits(cond, uncond, cfg_scale, mask, proc.eos_token_id if plan.eos_mode else None, plan.eos_mode,
                                 plan.temperature, penalty, seen, out=cond)
                u = torch.rand(B, device=dev) if sample else None
                toks = lmsample.pick(x, top_k, top_p, temperature, u)[0]
                stats["native_steps"] += 1
            else:
                cur = torch.cat([ids[:B], tokens[:step].t().to(ids.dtype)], dim=1)
                x = uncond + cfg_scale * (cond - uncond)
                x = proc(cur, x)
                for lp in handler._build_logits_processor(repetition_penalty):
                    x = lp(cur, x)
                toks = lmsample.select_tokens(x, top_k, top_p, temperature, check=False)
            tokens[step] = toks
            steps = step + 1
            if seen is not None:
                seen.mark(tokens[step])
            if plan.native and plan.sync_free:
                for _ in range(B):
                    proc.update_state(0)   # CODES_GENERATION only counts (update_state :2153-2158): the value is not looked at
                stats["sync_free_steps"] += 1
                continue
            host = toks.tolist()
            stats["token_reads"] += 1
            if min(host) < 0:
                bad_draw = True
                break
            if proc is not None:
                for t in host:
                    proc.update_state(t)
            if streamer is not None:
                streamer.put(toks.unsqueeze(1))
            if eos in host or (pad_token_id is not None and pad_token_id != eos and pad_token_id in host):
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
    return torch.cat([ids, tokens[:steps].t().repeat(2, 1).to(ids.dtype)], dim=1)
