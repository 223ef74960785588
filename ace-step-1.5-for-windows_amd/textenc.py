"""NativeTextEncoder: Python owner of an ``ace355_textenc`` handle - the reference's caption text encoder on the GPU.

The reference loads Qwen3-Embedding-0.6B with ``AutoModel.from_pretrained`` (init_service_loader.py:146-161), i.e. transformers'
``Qwen3Model``, and calls it twice (conditioning_embed.py:71-79):

* ``self.text_encoder(input_ids=ids, lyric_attention_mask=None).last_hidden_state`` for the right-padded caption ids, with no attention
  mask - so the stack is purely causal over the padded length, and the pad rows attend the prefix and the earlier pads;
* ``self.text_encoder.embed_tokens(lyric_ids)``: a row gather from the ``[vocab, hidden]`` table.

This class is call-compatible with both.  It is not an ``nn.Module``: the seam (``NativeTextEncoderMixin`` in backend.py) wraps it in
``modswap.NativeTextEncoderSwap``, which keeps the reference module as the fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Union

import torch

from . import native
from .config import TextEncoderConfig

_UNSUPPORTED_KWARGS = ("inputs_embeds", "past_key_values", "position_ids", "cache_position")


class TextEncoderOutput(tuple):
    """What callers read off ``Qwen3Model``'s output: ``.last_hidden_state`` (and ``[0]``, the same tensor)."""

    def __new__(cls, last_hidden_state: torch.Tensor):
        return super().__new__(cls, (last_hidden_state,))

    @property
    def last_hidden_state(self) -> torch.Tensor:
        return self[0]


def _host_ids(ids, vocab: int, what: str) -> torch.Tensor:
    """int32 CPU copy of the ids, range-checked (an id outside [0, vocab) is a ValueError before any native call)."""
    if not isinstance(ids, torch.Tensor):
        ids = torch.as_tensor(ids)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.is_complex():
        raise ValueError(f"ace355: {what} must be integer token ids, got {ids.dtype}")
    t = ids.detach().to("cpu")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= vocab):
        raise ValueError(f"ace355: {what} holds ids outside [0, {vocab}) (min {int(t.min())}, max {int(t.max())})")
    return t.to(torch.int32).contiguous()


class NativeTextEncoder(native.Owner):
    _destroy = "ace355_textenc_destroy"

    def __init__(self, cfg: TextEncoderConfig, device: Union[str, torch.device] = "cuda:0", out_dtype: torch.dtype = torch.bfloat16):
        self.cfg = cfg
        self.device = torch.device(device)
        self.out_dtype = out_dtype
        self._lib = native.lib()
        c = native.TextEncConfigC(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                                  cfg.num_key_value_heads, cfg.head_dim, cfg.vocab_size, cfg.rms_norm_eps, cfg.rope_theta)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.ace355_textenc_create(C.byref(c), C.byref(h))
        if rc == 4:   # ACE355_ERR_UNSUPPORTED
            raise NotImplementedError(f"ace355: {native.last_error()}")
        native.check(rc, "textenc_create")
        self._h = h

    @classmethod
    def from_reference(cls, module, device: Union[str, torch.device], out_dtype: torch.dtype = None) -> "NativeTextEncoder":
        """Build from the loaded ``Qwen3Model`` (``handler.text_encoder``): its config and its state_dict.  Output dtype: the module's."""
        if out_dtype is None:
            out_dtype = next(module.parameters()).dtype
        self = cls(TextEncoderConfig.from_reference(module.config), device, out_dtype)
        self.load_state_dict(module.state_dict())
        return self

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Keys of ``Qwen3Model.state_dict()``; rotary buffers are skipped."""
        native.load_state_dict(self._lib.ace355_textenc_load_tensor, self._lib.ace355_textenc_finalize, self._h, sd, "textenc",
                               self.device)

    def __call__(self, input_ids=None, attention_mask=None, *args, lyric_attention_mask=None, output_hidden_states=None,
                 output_attentions=None, use_cache=None, return_dict=None, **kwargs) -> TextEncoderOutput:
        """``Qwen3Model.forward`` for what the reference passes: ids [N, S] (CPU or GPU), no mask (or an all-ones one).
        ``lyric_attention_mask`` is accepted and ignored, as ``Qwen3Model`` ignores it."""
        if args:
            raise NotImplementedError("ace355: text encoder positional arguments beyond input_ids / attention_mask")
        for k in _UNSUPPORTED_KWARGS:
            if kwargs.pop(k, None) is not None:
                raise NotImplementedError(f"ace355: text encoder argument '{k}'")
        if kwargs:
            raise NotImplementedError(f"ace355: text encoder arguments {sorted(kwargs)}")
        if output_hidden_states or output_attentions:
            raise NotImplementedError("ace355: the native text encoder returns last_hidden_state only")
        if input_ids is None:
            raise NotImplementedError("ace355: the native text encoder needs input_ids")
        if input_ids.dim() != 2:
            raise ValueError("ace355: input_ids must be [batch, seq]")
        if attention_mask is not None and not bool(torch.all(attention_mask.detach().to("cpu") != 0)):
            raise NotImplementedError("ace355: the native text encoder runs without a padding mask (all-ones masks only)")
        ids = _host_ids(input_ids, self.cfg.vocab_size, "input_ids")
        N, S = ids.shape
        out = torch.empty(N, S, self.cfg.hidden_size, device=self.device, dtype=torch.bfloat16)
        if ids.numel():
            self._encode(ids, out)
        return TextEncoderOutput(out if self.out_dtype == torch.bfloat16 else out.to(self.out_dtype))

    forward = __call__

    def embed_tokens(self, ids) -> torch.Tensor:
        """``Qwen3Model.embed_tokens(ids)``: rows of the table, shape ``ids.shape + (hidden,)``, in the output dtype."""
        t = _host_ids(ids, self.cfg.vocab_size, "embed_tokens ids")
        out = torch.empty(*t.shape, self.cfg.hidden_size, device=self.device, dtype=torch.bfloat16)
        if t.numel():
            self._embed(t.reshape(-1), out)
        return out if self.out_dtype == torch.bfloat16 else out.to(self.out_dtype)

    # the two native calls (checked int32 host ids in, bf16 device rows out)
    def _encode(self, ids: torch.Tensor, out: torch.Tensor) -> None:
        N, S = ids.shape
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_textenc_encode(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int32)), N, S, native.ptr(out),
                                                          native.current_stream_ptr()), "textenc_encode")

    def _embed(self, ids: torch.Tensor, out: torch.Tensor) -> None:
        with torch.cuda.device(self.device):
            native.check(self._lib.ace355_textenc_embed(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int32)), ids.numel(),
                                                         native.ptr(out), native.current_stream_ptr()), "textenc_embed")
