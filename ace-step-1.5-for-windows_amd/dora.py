"""DoRA (weight decomposition) on top of the LoRA / LoKr merge terms of the native DiT.

A ``DoraTerm`` rescales the merged weight of one target, it is not an additive term: with ``V = W0 + sum of the target's LoraTerm /
KronTerm deltas`` (their scales holding the multiplier),

    n  = ||V||_2 over the row (``per_input`` False: one n, one g per output row) or over the column (``per_input`` True)
    f  = 1 + scale * (g / (n + eps) - 1)
    W' = V * f

(include/ace355.h ``ace355_dit_set_adapters_dora``).  LyCORIS ``LokrModule`` with ``wd``: ``g = dora_scale`` ([out, 1] or [1, in]),
``scale = multiplier``, ``eps = finfo(dora_scale.dtype).eps``.  PEFT ``use_dora``: ``g = lora_magnitude_vector`` [out], ``eps = 0``,
``scale = 1``.  Both are restated from the published modules; neither library is imported here nor part of the reference tree, so the
semantics are unpinned.  Where ``n + eps == 0`` (PEFT, an all-zero row) ``f = 1``; PEFT would produce NaN there.
"""
from __future__ import annotations

from typing import NamedTuple

import torch


class DoraTerm(NamedTuple):
    name: str              # reference key of the target weight
    g: torch.Tensor        # out (per_input False) or in (per_input True) magnitudes, any shape with that many elements
    per_input: bool        # the axis of the norm: False = per output row, True = per input column
    eps: float             # added to the norm (LyCORIS: finfo(dtype).eps; PEFT: 0)
    scale: float           # m of the interpolation (LyCORIS multiplier x the user's scale; PEFT: 1); 0 drops the term


def dora_eps(dtype: torch.dtype) -> float:
    """``torch.finfo(dtype).eps``, the LyCORIS epsilon for a ``dora_scale`` held in ``dtype`` (2^-7 for bf16)."""
    return float(torch.finfo(dtype).eps)


def axis_of(shape, out_f: int, in_f: int, what: str) -> bool:
    """``per_input`` from the shape of a LyCORIS ``dora_scale``: [out, 1] is the output axis, [1, in] the input axis."""
    shape = tuple(int(x) for x in shape)
    if shape == (out_f, 1):
        return False
    if shape == (1, in_f):
        return True
    raise ValueError(f"{what}: dora_scale {shape} is neither [{out_f}, 1] nor [1, {in_f}]")


def check_g(t: DoraTerm, out_f: int, in_f: int) -> None:
    n = in_f if t.per_input else out_f
    if t.g.numel() != n:
        raise ValueError(f"DoRA magnitudes for {t.name}: {tuple(t.g.shape)} does not hold the {n} values of the "
                         f"{'input' if t.per_input else 'output'} axis of [{out_f}, {in_f}]")
