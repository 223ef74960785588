"""NativeCausalLM: Python owner of an ``ace355_lm`` handle - the forward of the reference's 5 Hz LM on the GPU.

The LM is transformers' ``Qwen3ForCausalLM`` (0.6B / 1.7B; the 4B's 32 / 8 head layout with ``allow_gqa4=True``).  The reference's CFG loop (``_generate_with_cfg_custom``,
llm_inference.py:2414-2533) calls it through ``LLMHandler._forward_pass`` (llm_inference.py:416-438) in two ways:

* step 0: ``model(input_ids=ids[N, P], attention_mask=mask[N, P], use_cache=True)`` with left-padded rows (``0...0 1...1``);
* step t: ``model(input_ids=ids[:, -1:], past_key_values=<the previous step's>, attention_mask=mask[N, P + t], use_cache=True)``;

and reads ``outputs.logits[:, -1, :]`` and ``outputs.past_key_values`` only.  This class answers both: a native prefill that fills the
handle's KV cache, and a native one-row decode step, each returning the last column's logits.  No ``position_ids`` are passed, so
positions are the padded column indices and the first visible key of a row is its count of leading zeros.

Only the forward is native here.  By default the CFG combine, repetition penalty and the constrained logits processor stay the
reference's torch code, run on the logits returned here; top-k / top-p and the draw have a native counterpart in ``ace355.lmsample``
(opt-in at the seam: ``NativeLmMixin.use_native_lm_sampler``), and the rest of the loop body in ``ace355.lmlogits`` (opt-in:
``NativeLmMixin.use_native_lm_loop``), which drives ``decode_tokens`` below.  ``score`` is the teacher-forced counterpart for the
reference's quality score (``ace355.lmscore``; opt-in: ``NativeLmMixin.use_native_lm_score``): the prefill's pass, then per target token one
log-probability and one rank instead of logits.  It is not an ``nn.Module``: ``modswap.NativeCausalLMSwap`` wraps it and keeps
the reference module as the fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Union

import torch

from . import native
from .config import LmConfig
from .textenc import _host_ids

_UNSUPPORTED_KWARGS = ("inputs_embeds", "position_ids", "labels", "cache_position")


class KvToken:
    """``outputs.past_key_values`` of a native call: names the handle that holds the cache and the call that produced it.  Valid only
    as the token returned by the immediately preceding call of that handle."""

    __slots__ = ("owner", "generation")

    def __init__(self, owner: "NativeCausalLM", generation: int):
        self.owner = owner
        self.generation = generation


class CausalLMOutput:
    """What ``_forward_pass`` reads off ``Qwen3ForCausalLM``'s output: ``.logits`` ([N, 1, V]: the last column) and ``.past_key_values``."""

    __slots__ = ("logits", "past_key_values")

    def __init__(self, logits: torch.Tensor, past_key_values: KvToken):
        self.logits = logits
        self.past_key_values = past_key_values


def left_pad_first(attention_mask: torch.Tensor) -> List[int]:
    """Leading-zero count of every row of a ``0...0 1...1`` mask.  Holes, right pads and all-zero rows are ``NotImplementedError``:
    the native attention sees keys ``first[n] <= j <= i`` and nothing else."""
    m = attention_mask.detach().to("cpu")
    if m.dim() != 2 or m.shape[1] == 0:
        raise NotImplementedError("ace355: the LM's attention_mask must be [batch, positions]")
    m = m != 0
    ones = m.sum(1)
    first = m.shape[1] - ones
    if bool((ones == 0).any()):
        raise NotImplementedError("ace355: attention_mask row without a visible position")
    cols = torch.arange(m.shape[1])[None, :]
    if not bool((m == (cols >= first[:, None])).all()):
        raise NotImplementedError("ace355: the native LM takes left-padded masks (0...0 1...1 per row) only")
    return [int(v) for v in first]


class NativeCausalLM(native.Owner):
    _destroy = "ace355_lm_destroy"

    def __init__(self, cfg: LmConfig, device: Union[str, torch.device] = "cuda:0", max_positions: int = 8192,
                 max_seqs: int = native.LM_MAX_SEQS, out_dtype: torch.dtype = torch.float32, allow_gqa4: bool = False):
        """``allow_gqa4``: also take four q heads per kv head (Qwen3-4B's 32 / 8 layout) - ``ace355_lm_create_ex`` with
        ``ACE355_LM_ALLOW_GQA4``.  Without it the handle is created as ever and such a layout is ``NotImplementedError``."""
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # "cuda" (what LLMHandler.initialize stores) means the current device; tensors report theirs with an index, and
            # torch.device("cuda") != torch.device("cuda:0"), so the handle names the device it is really on
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.out_dtype = out_dtype
        self.max_positions, self.max_seqs = int(max_positions), int(max_seqs)
        self._generation = 0
        self._first: Optional[List[int]] = None
        self._lib = native.lib()
        c = native.LmConfigC(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                             cfg.num_key_value_heads, cfg.head_dim, cfg.vocab_size, cfg.rms_norm_eps, cfg.rope_theta,
                             1 if cfg.tie_word_embeddings else 0, self.max_seqs, self.max_positions)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if allow_gqa4:
                rc = self._lib.ace355_lm_create_ex(C.byref(c), native.LM_ALLOW_GQA4, C.byref(h))
            else:
                rc = self._lib.ace355_lm_create(C.byref(c), C.byref(h))
        if rc == 4:   # ACE355_ERR_UNSUPPORTED
            raise NotImplementedError(f"ace355: {native.last_error()}")
        native.check(rc, "lm_create")
        self._h = h

    @classmethod
    def from_reference(cls, module, device: Union[str, torch.device], out_dtype: torch.dtype = None,
                       max_positions: int = 8192, allow_gqa4: bool = False) -> "NativeCausalLM":
        """Build from the loaded ``Qwen3ForCausalLM`` (``LLMHandler.llm``): its config and its state_dict.  Logits dtype: the module's.
        ``allow_gqa4``: as in the constructor."""
        if out_dtype is None:
            out_dtype = next(module.parameters()).dtype
        self = cls(LmConfig.from_reference(module.config, allow_gqa4=allow_gqa4), device, max_positions=max_positions, out_dtype=out_dtype,
                   allow_gqa4=allow_gqa4)
        self.load_state_dict(module.state_dict())
        return self

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Keys of ``Qwen3ForCausalLM.state_dict()``; rotary buffers are skipped.  A tied checkpoint's ``lm_head.weight`` is dropped by
        the library (it is the embedding table)."""
        native.load_state_dict(self._lib.ace355_lm_load_tensor, self._lib.ace355_lm_finalize, self._h, sd, "lm", self.device)

    @property
    def length(self) -> int:
        """Positions the cache holds (0 before the first prefill)."""
        return self._length()

    # ------------------------------------------------------------------ the two steps: fp32 [N, V] logits of the last column
    def _prompt(self, ids, attention_mask):
        """What ``prefill`` and ``score`` check alike: ``(ids as a [N, P] tensor, first)`` for a prompt the handle can take."""
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.shape[1] == 0 or ids.shape[0] == 0:
            raise ValueError("ace355: input_ids must be a non-empty [batch, positions]")
        N, P = ids.shape
        if attention_mask is None:
            first = [0] * N
        else:
            if tuple(attention_mask.shape) != (N, P):
                raise NotImplementedError(f"ace355: attention_mask {tuple(attention_mask.shape)} for input_ids {(N, P)}")
            first = left_pad_first(attention_mask)
        if N > self.max_seqs or P > self.max_positions or N * P > native.LM_MAX_TOKENS:
            raise ValueError(f"ace355: an LM prefill of {N} x {P} exceeds the handle ({self.max_seqs} sequences, {self.max_positions} "
                             f"positions, {native.LM_MAX_TOKENS} tokens)")
        return ids, first

    def _decode_seqs(self) -> int:
        """The state ``decode`` and ``decode_tokens`` need: a prefill to continue from and room for one more position.  Returns N."""
        if self._first is None:
            raise ValueError("ace355: LM decode without a prefill")
        if self.length >= self.max_positions:
            raise ValueError(f"ace355: the LM cache is full ({self.max_positions} positions)")
        return len(self._first)

    def prefill(self, ids, attention_mask=None) -> torch.Tensor:
        ids, first = self._prompt(ids, attention_mask)
        N = ids.shape[0]
        host = _host_ids(ids, self.cfg.vocab_size, "input_ids")
        out = torch.empty(N, self.cfg.vocab_size, device=self.device, dtype=torch.float32)
        self._generation += 1
        self._first = None
        self._prefill(host, torch.tensor(first, dtype=torch.int32), out)
        self._first = first
        return out

    def score(self, ids, attention_mask=None, start=None):
        """Teacher-forced scoring (``ace355_lm_score``): for every sequence ``n`` and column ``c`` in ``[start[n], P)`` the log-probability
        of ``ids[n][c]`` given the columns before it, and its 0-based rank among that position's logits (0: it is the argmax; equal
        logits are ordered by ascending id).  ``start``: an int or one per sequence, ``first[n] < start[n] < P``.  Returns
        ``(logprob fp32 [R], rank int32 [R])`` on the device, compact in ``(n, c)`` order.  Refuses what ``prefill`` refuses; it is not a
        prefill: afterwards the handle holds no generation, a ``decode`` raises and an older ``KvToken`` is stale."""
        ids, first = self._prompt(ids, attention_mask)
        N, P = ids.shape
        if start is None:
            raise ValueError("ace355: LM score needs start (the first scored column of every sequence)")
        start = [int(start)] * N if isinstance(start, int) else [int(v) for v in start]
        if len(start) != N or any(not f < s < P for f, s in zip(first, start)):
            raise ValueError(f"ace355: LM score start {start} must lie in (first, P) = ({first}, {P}) for each of the {N} sequences")
        host = _host_ids(ids, self.cfg.vocab_size, "input_ids")
        R = sum(P - s for s in start)
        logprob = torch.empty(R, device=self.device, dtype=torch.float32)
        rank = torch.empty(R, device=self.device, dtype=torch.int32)
        self._generation += 1
        self._first = None
        p32 = C.POINTER(C.c_int32)
        first_t, start_t = torch.tensor(first, dtype=torch.int32), torch.tensor(start, dtype=torch.int32)
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_lm_score(self._h, C.cast(host.data_ptr(), p32), C.cast(first_t.data_ptr(), p32),
                                                   C.cast(start_t.data_ptr(), p32), N, P, native.ptr(logprob), native.ptr(rank),
                                                   native.current_stream_ptr()), "lm_score")
        return logprob, rank

    def decode(self, next_ids) -> torch.Tensor:
        if not isinstance(next_ids, torch.Tensor):
            next_ids = torch.as_tensor(next_ids)
        N = self._decode_seqs()
        if next_ids.numel() != N or next_ids.dim() > 2 or (next_ids.dim() == 2 and next_ids.shape[1] != 1):
            raise ValueError(f"ace355: LM decode takes one token for each of the {N} sequences")
        host = _host_ids(next_ids.reshape(-1), self.cfg.vocab_size, "input_ids")
        out = torch.empty(N, self.cfg.vocab_size, device=self.device, dtype=torch.float32)
        self._generation += 1
        self._decode(host, out)
        return out

    def decode_tokens(self, tokens: torch.Tensor) -> torch.Tensor:
        """``decode`` for ids that stay on the GPU: ``tokens`` int64 ``[B]`` on this device, ``N % B == 0``, sequence ``n`` takes
        ``tokens[n % B]`` (the CFG loop's ``next_tokens.repeat(2, 1)``).  Nothing is read back and the stream is not synchronised; an id
        outside the vocabulary is embedded as id 0 and counted (``bad_tokens``)."""
        N = self._decode_seqs()
        if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.device != self.device or tokens.dim() != 1:
            raise ValueError(f"ace355: decode_tokens takes an int64 [B] tensor on {self.device}")
        B = tokens.shape[0]
        if B < 1 or N % B != 0:
            raise ValueError(f"ace355: {B} tokens for {N} sequences (N must be a multiple of B)")
        if not tokens.is_contiguous():
            tokens = tokens.contiguous()
        out = torch.empty(N, self.cfg.vocab_size, device=self.device, dtype=torch.float32)
        self._generation += 1
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_lm_decode_tokens(self._h, tokens.data_ptr(), B, native.ptr(out), native.current_stream_ptr()),
                         "lm_decode_tokens")
        return out

    def fan_out(self, src) -> None:
        """``ace355_lm_fan_out``: the cache's sequences become ``len(src)`` sequences of the same length, sequence ``n`` a copy of
        old sequence ``src[n]`` (``src`` non-decreasing, ``src[n] <= n``).  B songs with one prompt: prefill the ``[2, P]`` pair, then
        ``fan_out([0] * B + [1] * B)``.  In place, on the current stream, nothing is read back; tokens of earlier calls go stale."""
        if self._first is None:
            raise ValueError("ace355: LM fan-out without a prefill")
        src = [int(v) for v in src]
        n_old = len(self._first)
        if not 1 <= len(src) <= self.max_seqs:
            raise ValueError(f"ace355: a fan-out to {len(src)} sequences, the handle holds 1 .. {self.max_seqs}")
        if any(s > n or s >= n_old or s < 0 or (n and s < src[n - 1]) for n, s in enumerate(src)):
            raise ValueError(f"ace355: fan-out src {src} must be non-decreasing with src[n] <= n and src[n] < {n_old}")
        arr = (C.c_int32 * len(src))(*src)
        self._generation += 1
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_lm_fan_out(self._h, arr, len(src), native.current_stream_ptr()), "lm_fan_out")
        self._first = [self._first[s] for s in src]

    def bad_tokens(self) -> int:
        """Out-of-vocabulary ids ``decode_tokens`` has replaced since the last call of this method (one synchronisation; clears)."""
        with torch.cuda.device(self.device):
            n = int(self._lib.ace355_lm_bad_tokens(self._h))
        if n < 0:
            raise RuntimeError(f"ace355 native call failed (lm_bad_tokens): {native.last_error()}")
        return n

    # ------------------------------------------------------------------ Qwen3ForCausalLM.forward for what _forward_pass passes
    def __call__(self, input_ids=None, attention_mask=None, past_key_values=None, use_cache=True, *args, output_hidden_states=None,
                 output_attentions=None, logits_to_keep=0, return_dict=None, **kwargs) -> CausalLMOutput:
        if args:
            raise NotImplementedError("ace355: LM positional arguments beyond input_ids / attention_mask / past_key_values / use_cache")
        for k in _UNSUPPORTED_KWARGS:
            if kwargs.pop(k, None) is not None:
                raise NotImplementedError(f"ace355: LM argument '{k}'")
        if kwargs:
            raise NotImplementedError(f"ace355: LM arguments {sorted(kwargs)}")
        if output_hidden_states or output_attentions:
            raise NotImplementedError("ace355: the native LM returns logits and its cache token only")
        if isinstance(logits_to_keep, torch.Tensor) or logits_to_keep not in (0, 1):
            raise NotImplementedError("ace355: the native LM computes the last column's logits only (logits_to_keep 0 / 1)")
        if input_ids is None or input_ids.dim() != 2:
            raise NotImplementedError("ace355: the native LM needs input_ids [batch, positions]")
        if past_key_values is None:
            logits = self.prefill(input_ids, attention_mask)
        else:
            if not isinstance(past_key_values, KvToken) or past_key_values.owner is not self:
                raise NotImplementedError("ace355: past_key_values is not this native LM's cache token")
            if past_key_values.generation != self._generation or self._first is None:
                raise NotImplementedError("ace355: stale cache token (only the previous call's past_key_values continues a generation)")
            N, L = len(self._first), self.length
            if tuple(input_ids.shape) != (N, 1):
                raise NotImplementedError(f"ace355: a native decode step takes input_ids [{N}, 1], got {tuple(input_ids.shape)}")
            if attention_mask is not None:
                if tuple(attention_mask.shape) != (N, L + 1):
                    raise NotImplementedError(f"ace355: attention_mask {tuple(attention_mask.shape)} at cache length {L} (expected {(N, L + 1)})")
                if left_pad_first(attention_mask) != self._first:
                    raise NotImplementedError("ace355: the attention_mask's padding differs from the prefill's")
            logits = self.decode(input_ids)
        logits = logits[:, None, :]
        return CausalLMOutput(logits if self.out_dtype == torch.float32 else logits.to(self.out_dtype), KvToken(self, self._generation))

    forward = __call__

    # the native calls (checked int32 host ids in, fp32 device logits out)
    def _prefill(self, ids: torch.Tensor, first: torch.Tensor, out: torch.Tensor) -> None:
        N, P = ids.shape
        p32 = C.POINTER(C.c_int32)
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_lm_prefill(self._h, C.cast(ids.data_ptr(), p32), C.cast(first.data_ptr(), p32), N, P,
                                                     native.ptr(out), native.current_stream_ptr()), "lm_prefill")

    def _decode(self, ids: torch.Tensor, out: torch.Tensor) -> None:
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_lm_decode(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int32)), native.ptr(out),
                                                    native.current_stream_ptr()), "lm_decode")

    def _length(self) -> int:
        return int(self._lib.ace355_lm_length(self._h))
