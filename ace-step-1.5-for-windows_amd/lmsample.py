"""Token selection on the 5 Hz LM's logits, on the GPU: top-k, top-p and the draw in one native call (``ace355_lm_pick``).

The reference does this at one seam, three ``LLMHandler`` methods called in a row on the same ``[B, V]`` tensor
(``_apply_top_k_filter``, ``_apply_top_p_filter``, ``_sample_tokens``; llm_inference.py:367-399): a ``torch.topk``, a full descending
``torch.sort`` of every row, two softmaxes, a cumsum, a scatter and a ``torch.multinomial``.  ``select_tokens`` computes the same keep
set without a sort (radix selection, csrc/lm_sample.hip) and draws from the same distribution ``softmax(filtered / T)`` by inverse CDF
with one uniform ``u`` per row.  The draw for a given seed is not ``torch.multinomial``'s, so ``NativeLmMixin`` uses this only when
asked to (``use_native_lm_sampler``).  Semantics, exactly: include/ace355.h above ``ace355_lm_pick``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import torch

from . import native

MAX_ROWS = native.LM_MAX_SEQS   # rows of one native call; more are run in slices


def _rows_f32(logits: torch.Tensor) -> torch.Tensor:
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("ace355: logits must be [B, V] with B, V >= 1")
    if not logits.is_cuda:
        raise ValueError("ace355: logits must be on the GPU (there is no CPU fallback)")
    if logits.shape[1] > native.LM_PICK_MAX_V:
        raise ValueError(f"ace355: at most {native.LM_PICK_MAX_V} logits per row")
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.float()   # as the reference upcasts before its softmax
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def pick(logits: torch.Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: float = 1.0,
         u: Optional[torch.Tensor] = None, want_kept: bool = False, want_mask: bool = False):
    """The native call as it is: returns ``(tokens int64 [B], kept int32 [B] or None, keep uint8 [B, V] or None)``.  A row with a NaN, a
    ``+inf`` or no finite entry has token -1, kept 0 and an all-zero mask.  ``u``: fp32 ``[B]`` in [0, 1), required for
    ``temperature > 0``.  The logits are only read; everything runs on the current stream."""
    x = _rows_f32(logits)
    B, V = x.shape
    dev = x.device
    k = int(top_k) if top_k is not None and top_k > 0 else 0
    p = float(top_p) if top_p is not None and 0.0 < top_p < 1.0 else 0.0
    T = float(temperature)
    params = native.LmPickParamsC(top_k=min(k, 2 ** 31 - 1), top_p=p, temperature=T, reserved=0)
    if T > 0:
        if u is None:
            raise ValueError("ace355: u is required when temperature > 0")
        u = u.detach().to(device=dev, dtype=torch.float32).contiguous()
        if u.shape != (B,):
            raise ValueError("ace355: u must hold one value per row")
    lib = native.lib()
    with torch.cuda.device(dev):
        tokens = torch.empty(B, dtype=torch.int64, device=dev)
        kept = torch.empty(B, dtype=torch.int32, device=dev) if want_kept else None
        keep = torch.empty(B, V, dtype=torch.uint8, device=dev) if want_mask else None
        n0 = min(B, MAX_ROWS)
        ws_bytes = int(lib.ace355_lm_pick_workspace_bytes(n0, V))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)   # (the caching allocator ties it to the current stream)
        stream = native.current_stream_ptr()
        for r0 in range(0, B, MAX_ROWS):
            n = min(MAX_ROWS, B - r0)
            native.check(lib.ace355_lm_pick(x[r0].data_ptr(), x.stride(0), n, V, C.byref(params), u[r0:].data_ptr() if T > 0 else None,
                                            tokens[r0:].data_ptr(), kept[r0:].data_ptr() if want_kept else None,
                                            keep[r0].data_ptr() if want_mask else None, ws.data_ptr(), ws_bytes, stream), "lm_pick")
    return tokens, kept, keep


def select_tokens(logits: torch.Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: float = 1.0,
                  u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, return_mask: bool = False,
                  check: bool = True) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``_apply_top_k_filter`` -> ``_apply_top_p_filter`` -> ``_sample_tokens`` on ``logits`` ([B, V] on the GPU, rows may be strided;
    not modified) as one native call: int64 tokens ``[B]``, with ``return_mask`` also the bool keep mask ``[B, V]``.

    ``temperature <= 0`` is greedy.  Otherwise one uniform per row decides the draw: ``u`` (fp32 ``[B]`` in [0, 1)), by default
    ``torch.rand(B, device=..., generator=generator)``, so ``torch.manual_seed`` governs it as it governs ``torch.multinomial`` - the
    distribution is the reference's, the draw for a given seed is not.  ``check`` raises ``RuntimeError`` when a row had a NaN, a ``+inf``
    or no finite entry (token -1); that is one synchronisation, which the reference's loop pays anyway when it reads the token."""
    if temperature > 0 and u is None:
        u = torch.rand(logits.shape[0], device=logits.device, generator=generator)
    tokens, _kept, keep = pick(logits, top_k, top_p, temperature, u, want_mask=return_mask)
    if check and bool((tokens < 0).any()):
        bad = torch.nonzero(tokens < 0).flatten().tolist()
        raise RuntimeError(f"ace355: logits rows {bad} hold a NaN, a +inf or no finite entry; no token can be selected")
    return (tokens, keep.bool()) if return_mask else tokens


def filter_logits_(logits: torch.Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None) -> torch.Tensor:
    """What the reference's two filters do together, in place: every entry the keep mask drops becomes ``-inf``.  Returns ``logits``."""
    _tokens, _kept, keep = pick(logits, top_k, top_p, 0.0, None, want_mask=True)
    logits.masked_fill_(keep == 0, float("-inf"))
    return logits
