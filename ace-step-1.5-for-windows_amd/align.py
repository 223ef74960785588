"""Lyric alignment on the native DiT: the cross-attention maps the reference's ``get_lyric_timestamp`` / ``get_lyric_score`` read.

The reference runs the decoder with ``output_attentions=True`` (H/lyric_timestamp.py:78, H/lyric_score.py:97; H = acestep/core/
generation/handler) and hands the probabilities of the (layer, head) pairs of ``custom_layers_config`` to its aligners.  Here the maps come
from ``NativeDit.cross_attention_maps`` (one eager call that stops after the last requested layer) and are laid out as the handlers lay
them out, so the host's aligners (``acestep.core.scoring``) consume them unchanged.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

# acestep/handler.py:129
DEFAULT_LAYERS_HEADS: Dict[int, List[int]] = {2: [6], 3: [10, 11], 4: [3], 5: [8, 9], 6: [8]}

KINDS = ("timestamp", "score")


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def pairs(config: Dict[int, Sequence[int]], cfg) -> List[Tuple[int, int]]:
    """The (layer, head) pairs of a ``custom_layers_config``, sorted and without duplicates.  ``cfg``: the DiT's ``DitConfig``."""
    if not config:
        raise ValueError("custom_layers_config is empty: no (layer, head) pair to capture")
    out = set()
    for layer, heads in config.items():
        if not _is_int(layer) or not 0 <= layer < cfg.num_hidden_layers:
            raise ValueError(f"custom_layers_config: layer {layer!r} is not an integer in [0, {cfg.num_hidden_layers})")
        if isinstance(heads, (str, bytes)) or not hasattr(heads, "__iter__"):
            raise ValueError(f"custom_layers_config: layer {layer} maps to {heads!r}, not a list of heads")
        for hd in heads:
            if not _is_int(hd) or not 0 <= hd < cfg.num_attention_heads:
                raise ValueError(f"custom_layers_config: head {hd!r} of layer {layer} is not an integer in [0, {cfg.num_attention_heads})")
            out.add((layer, hd))
    if not out:
        raise ValueError("custom_layers_config names no head")
    return sorted(out)


def noise_like(pred_latent: torch.Tensor, seed: Optional[int]) -> torch.Tensor:
    """``_sample_noise_like`` (H/lyric_alignment_common.py:36-48): a generator on the latent's device seeded with ``seed``, ``randn`` in
    the latent's dtype; ``randn_like`` without a seed."""
    if seed is None:
        return torch.randn_like(pred_latent)
    g = torch.Generator(device=pred_latent.device).manual_seed(int(seed))
    return torch.randn(pred_latent.shape, generator=g, device=pred_latent.device, dtype=pred_latent.dtype)


def check_steps(inference_steps) -> float:
    if not isinstance(inference_steps, int) or inference_steps <= 0:
        raise ValueError(f"inference_steps must be a positive non-zero integer, got {inference_steps!r}")
    return 1.0 / inference_steps


def alignment_rows(pred_latent: torch.Tensor, noise: torch.Tensor, inference_steps: int, kind: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Decoder rows and timesteps of one alignment call, in the latent's dtype as the reference computes them.
    ``"timestamp"`` (H/lyric_timestamp.py:71-75): ``x = t noise + (1 - t) pred``, t = 1 / inference_steps.
    ``"score"`` (H/lyric_score.py:70-89): ``[noise at t = 1 ; t noise + (1 - t) pred at t]``, 2 B rows."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    t_last = check_steps(inference_steps)
    bsz = pred_latent.shape[0]
    xt = t_last * noise + (1.0 - t_last) * pred_latent
    t = torch.tensor([t_last] * bsz, device=pred_latent.device, dtype=pred_latent.dtype)
    if kind == "timestamp":
        return xt, t
    ones = torch.tensor([1.0] * bsz, device=pred_latent.device, dtype=pred_latent.dtype)
    return torch.cat([noise, xt], 0), torch.cat([ones, t], 0)


def stack(maps: torch.Tensor, prs: Sequence[Tuple[int, int]], bsz: int, H: int, dtype: torch.dtype = torch.bfloat16
          ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """The handlers' layout of ``maps`` [n_pairs, N, L, S]: ``[max_layer + 1, N, H, L, S]`` in ``dtype`` (in bf16 the cast is the
    reference's ``.to(query.dtype)``), zeros outside the requested pairs.  N == bsz (timestamp): one stack; N == 2 bsz (score): the
    (lm, dit) pair of stacks, rows [:bsz] and [bsz:].  Each is squeezed to [layers, H, L, S] when bsz == 1 (H/lyric_timestamp.py:97-105,
    H/lyric_score.py:116-128); with bsz > 1 it keeps the item axis, as the reference does."""
    P, N, L, S = maps.shape
    if P != len(prs):
        raise ValueError(f"{P} maps for {len(prs)} pairs")
    full = torch.zeros(max(l for l, _ in prs) + 1, N, H, L, S, device=maps.device, dtype=dtype)
    for i, (l, hd) in enumerate(prs):
        full[l, :, hd] = maps[i].to(dtype)

    def squeeze(x):
        return x.squeeze(1) if bsz == 1 else x
    if N == bsz:
        return squeeze(full)
    if N == 2 * bsz:
        return squeeze(full[:, :bsz]), squeeze(full[:, bsz:])
    raise ValueError(f"maps of {N} rows do not fit a batch of {bsz}")


def lyric_maps(dit, pred_latent: torch.Tensor, encoder_hidden_states: torch.Tensor, context_latents: torch.Tensor,
               inference_steps: int = 8, seed: Optional[int] = 42, layers_heads: Optional[Dict[int, Sequence[int]]] = None,
               kind: str = "timestamp", dtype: torch.dtype = torch.bfloat16) -> Tuple[torch.Tensor, List[Tuple[int, int]], int]:
    """The fp32 maps [n_pairs, N, L, S] of one alignment call as ``NativeDit.cross_attention_maps`` returns them, with the sorted pairs
    and the batch size: N == bsz for ``"timestamp"``, 2 bsz for ``"score"`` (the lm rows, then the dit rows).  The inputs move to the
    DiT's device in ``dtype``, as the reference moves them to ``self.device`` / ``self.dtype`` (H/lyric_alignment_common.py:19-34).
    Item b's condition goes to slot b (slots [0, bsz)); the next request sets its slots again."""
    prs = pairs(layers_heads if layers_heads is not None else DEFAULT_LAYERS_HEADS, dit.cfg)
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    check_steps(inference_steps)
    dev = dit.device
    pred = pred_latent.to(device=dev, dtype=dtype)
    enc = encoder_hidden_states.to(device=dev, dtype=dtype)
    ctx = context_latents.to(device=dev, dtype=dtype)
    bsz = pred.shape[0]
    noise = noise_like(pred, seed)
    x, t = alignment_rows(pred, noise, inference_steps, kind)
    for b in range(bsz):
        dit.set_condition(b, enc[b if enc.shape[0] > 1 else 0])
    slots = list(range(bsz))
    if kind == "score":
        slots = slots * 2
        ctx = torch.cat([ctx, ctx], 0)
    tl = t.float().tolist()
    return dit.cross_attention_maps(x.float(), ctx.float(), tl, tl, slots, prs), prs, bsz


def lyric_attention(dit, pred_latent: torch.Tensor, encoder_hidden_states: torch.Tensor, context_latents: torch.Tensor,
                    inference_steps: int = 8, seed: Optional[int] = 42, layers_heads: Optional[Dict[int, Sequence[int]]] = None,
                    kind: str = "timestamp", dtype: torch.dtype = torch.bfloat16):
    """The maps of one ``get_lyric_timestamp`` (``kind="timestamp"``) or ``get_lyric_score`` (``"score"``, a (lm, dit) pair) call on the
    native DiT ``dit`` (``lyric_maps``), in the handlers' layout and ``dtype``."""
    maps, prs, bsz = lyric_maps(dit, pred_latent, encoder_hidden_states, context_latents, inference_steps, seed, layers_heads, kind, dtype)
    return stack(maps, prs, bsz, dit.cfg.num_attention_heads, dtype)
