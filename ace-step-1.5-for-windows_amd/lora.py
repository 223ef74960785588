"""PEFT LoRA adapters for the native DiT: read them from disk or from a PEFT-wrapped decoder as merge terms.

The reference trains and loads PEFT LoRA adapters on the decoder's attention and MLP projections (acestep/training/configs.py:22-27,
core/generation/handler/lora/lifecycle.py) and scales them through ``scaling[adapter]`` (core/lora/scaling.py:52).  PEFT's unmerged eval
forward ``y = x W^T + scaling * (x A^T) B^T`` equals a forward with ``W + scaling * B A``; the native handle merges exactly that into its
packed bf16 weights (``NativeDit.set_adapters``, include/ace355.h ``ace355_dit_set_adapters``).  One term = ``(name, A, B, scale)`` for
one adapter on one target weight, ``name`` the reference key of the target (``layers.3.cross_attn.k_proj.weight``).

LoKr (LyCORIS) adapters are the other family the handle merges: ``ace355.lokr``.
What the merge does not cover raises ``UnsupportedAdapter``, which the seam turns into the PyTorch path: adapters
with trained biases, ``modules_to_save``, ``fan_in_fan_out``, already merged PEFT modules, and targets outside the ten projection kinds.
DoRA (``use_dora``) is merged too, but it is not an additive term: the readers return it as ``ace355.dora.DoraTerm`` only to a caller
that asks with ``allow_dora=True`` and refuse it otherwise.
This module needs neither ``peft`` nor ``lycoris`` (it reads the attributes the reference itself reads,
core/lora/introspection.py:77-90).
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import Dict, List, NamedTuple, Optional

import torch

from .dora import DoraTerm, check_g

TARGET_KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                "cross_attn.q_proj", "cross_attn.k_proj", "cross_attn.v_proj", "cross_attn.o_proj",
                "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
_TARGET = re.compile(r"^layers\.(\d+)\.(" + "|".join(re.escape(k) for k in TARGET_KINDS) + r")$")
_PREFIXES = ("base_model.model.", "base_model.")
LOKR_WEIGHTS_FILENAME = "lokr_weights.safetensors"   # core/generation/handler/lora/lifecycle.py (LoKr artifact)


class UnsupportedAdapter(RuntimeError):
    """The adapter is valid but the native merge does not implement it: the PyTorch path must run it."""


class LoraTerm(NamedTuple):
    name: str              # reference key of the target weight
    A: torch.Tensor        # lora_A.weight [rank, in]
    B: torch.Tensor        # lora_B.weight [out, rank]
    scale: float           # PEFT scaling[adapter] (x the user's scale where the caller applies one)


def _module_path(name: str) -> str:
    for p in _PREFIXES:
        if name.startswith(p):
            return name[len(p):]
    return name


def _target_name(module: str, num_layers: Optional[int] = None) -> str:
    m = _TARGET.match(module)
    if m is None or (num_layers is not None and int(m.group(1)) >= num_layers):
        raise UnsupportedAdapter(f"LoRA target '{module}' is outside the projections the native DiT merges "
                                 "(layers.{i}.{self_attn,cross_attn}.{q,k,v,o}_proj, layers.{i}.mlp.{gate,up,down}_proj)")
    return module + ".weight"


def _check_shapes(terms: List[LoraTerm], cfg) -> None:
    if cfg is None:
        return
    shapes = cfg.weight_shapes()
    for t in terms:
        out_f, in_f = shapes[t.name]
        if t.A.dim() != 2 or t.B.dim() != 2 or t.A.shape[1] != in_f or t.B.shape[0] != out_f or t.A.shape[0] != t.B.shape[1] \
                or t.A.shape[0] < 1:
            raise ValueError(f"LoRA shapes for {t.name}: A {tuple(t.A.shape)}, B {tuple(t.B.shape)} do not fit the weight "
                             f"[{out_f}, {in_f}] of this configuration")


def _pattern_value(patterns: Dict[str, object], module: str, default):
    """PEFT's rank_pattern / alpha_pattern rule: the first pattern that the module name ends with, at a dot boundary."""
    for pat, v in (patterns or {}).items():
        if module == pat or module.endswith("." + pat):
            return v
    return default


def peft_scaling(alpha: float, r: int, use_rslora: bool) -> float:
    """LoraLayer.update_layer: lora_alpha / r, or lora_alpha / sqrt(r) with rsLoRA."""
    return float(alpha) / (math.sqrt(r) if use_rslora else float(r))


def read_peft_adapter(path: str, cfg=None, allow_dora: bool = False) -> list:
    """Terms (CPU tensors) of the PEFT LoRA directory ``path``: ``adapter_config.json`` + ``adapter_model.safetensors`` (or
    ``adapter_model.bin``).  ``cfg`` (a ``DitConfig``) checks every target's shape.  A ``use_dora`` adapter (the flag with a
    ``lora_magnitude_vector`` per module; one without the other is refused) needs ``allow_dora=True`` and adds one ``DoraTerm`` per
    module behind the ``LoraTerm`` list: the output axis, ``eps`` 0, ``scale`` 1."""
    if os.path.exists(os.path.join(path, LOKR_WEIGHTS_FILENAME)):
        raise UnsupportedAdapter("LoKr adapter (lokr_weights.safetensors): not merged natively")
    cfg_file = os.path.join(path, "adapter_config.json")
    if not os.path.exists(cfg_file):
        raise ValueError(f"expected a PEFT LoRA directory containing adapter_config.json: {path}")
    with open(cfg_file) as f:
        ac = json.load(f)
    if str(ac.get("peft_type", "LORA")).upper() != "LORA":
        raise UnsupportedAdapter(f"PEFT adapter type {ac.get('peft_type')}: only LoRA is merged natively")
    if ac.get("use_dora") and not allow_dora:
        raise UnsupportedAdapter("DoRA adapter: not merged natively")
    if ac.get("bias", "none") != "none" or ac.get("lora_bias"):
        raise UnsupportedAdapter("adapter with trained biases: not merged natively")
    if ac.get("modules_to_save"):
        raise UnsupportedAdapter("adapter with modules_to_save: not merged natively")
    if ac.get("fan_in_fan_out"):
        raise UnsupportedAdapter("fan_in_fan_out adapter: not merged natively")
    st = os.path.join(path, "adapter_model.safetensors")
    if os.path.exists(st):
        from safetensors import safe_open
        from safetensors.torch import load_file
        with safe_open(st, framework="pt") as f:
            meta = f.metadata() or {}
        if "lokr_config" in meta:
            raise UnsupportedAdapter("LoKr adapter (lokr_config metadata): not merged natively")
        sd = load_file(st)
    elif os.path.exists(os.path.join(path, "adapter_model.bin")):
        sd = torch.load(os.path.join(path, "adapter_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise ValueError(f"no adapter_model.safetensors / adapter_model.bin in {path}")
    r0, a0, rs = int(ac.get("r", 8)), float(ac.get("lora_alpha", 8)), bool(ac.get("use_rslora", False))
    parts: Dict[str, Dict[str, torch.Tensor]] = {}
    key_re = re.compile(r"^(.*)\.lora_([AB])(?:\.([^.]+))?\.weight$")
    mag_re = re.compile(r"^(.*)\.lora_magnitude_vector(?:\.([^.]+))?$")   # a parameter (older PEFT) or a module's .weight (newer)
    for key, t in sd.items():
        if "lora_magnitude_vector" in key:
            if not allow_dora:
                raise UnsupportedAdapter("DoRA adapter (lora_magnitude_vector): not merged natively")
            m = mag_re.match(key[:-len(".weight")] if key.endswith(".weight") else key)
            if m is None:
                raise UnsupportedAdapter(f"adapter tensor '{key}' is not a DoRA magnitude vector")
            parts.setdefault(_module_path(m.group(1)), {})["g"] = t
            continue
        m = key_re.match(key)
        if m is None:
            raise UnsupportedAdapter(f"adapter tensor '{key}' is not a LoRA A / B weight")
        module = _module_path(m.group(1))
        slot = parts.setdefault(module, {})
        slot[m.group(2)] = t
    terms, dora = [], []
    for module, ab in parts.items():
        if "A" not in ab and "B" not in ab:
            raise UnsupportedAdapter(f"DoRA magnitude vector for {module}, which has no lora_A / lora_B pair: not merged natively")
        if ("g" in ab) != bool(ac.get("use_dora")):
            raise UnsupportedAdapter(f"LoRA module {module}: use_dora and a lora_magnitude_vector belong together; "
                                     f"{'the vector is missing' if ac.get('use_dora') else 'adapter_config.json does not set use_dora'}")
        if not {"A", "B"} <= set(ab):
            raise ValueError(f"LoRA module {module} lacks its lora_{'A' if 'A' not in ab else 'B'} weight")
        name = _target_name(module, getattr(cfg, "num_hidden_layers", None))
        r = int(_pattern_value(ac.get("rank_pattern"), module, r0))
        alpha = float(_pattern_value(ac.get("alpha_pattern"), module, a0))
        if ab["A"].shape[0] != r:
            raise ValueError(f"LoRA module {module}: rank {ab['A'].shape[0]} in the weights, {r} in adapter_config.json")
        terms.append(LoraTerm(name, ab["A"], ab["B"], peft_scaling(alpha, r, rs)))
        if "g" in ab:
            dora.append(DoraTerm(name, ab["g"], False, 0.0, 1.0))
            check_g(dora[-1], int(ab["B"].shape[0]), int(ab["A"].shape[1]))
    _check_shapes(terms, cfg)
    return terms + dora


def _active(mod) -> List[str]:
    act = getattr(mod, "active_adapters", None)
    if act is None:
        act = getattr(mod, "active_adapter", None)
    if act is None:
        return []
    return [act] if isinstance(act, str) else list(act)


def _magnitude(mod, a):
    """``lora_magnitude_vector[a]`` of a PEFT module: a module with a ``.weight`` (newer PEFT) or the parameter itself (older)."""
    mv = getattr(mod, "lora_magnitude_vector", None)
    if mv is None or a not in mv:
        return None
    g = mv[a]
    return getattr(g, "weight", g)


def terms_from_decoder(decoder, cfg=None, allow_dora: bool = False) -> list:
    """Terms of a PEFT-wrapped decoder, by duck typing (no ``peft`` import): every module with ``lora_A`` / ``lora_B`` / ``scaling``
    whose adapters are enabled contributes ``scaling[a]``, ``lora_A[a].weight``, ``lora_B[a].weight`` for each active adapter ``a``.
    A LyCORIS network on the decoder (``_lycoris_net``) contributes its LoKr modules as ``ace355.lokr.KronTerm``, ahead of them.
    Weight-decomposed modules (LyCORIS ``wd``, PEFT ``use_dora``) need ``allow_dora=True`` and add their ``DoraTerm`` at the end."""
    terms: list = []
    dora: list = []
    net = getattr(decoder, "_lycoris_net", None)
    if net is not None:   # LoKr (H/lora/lifecycle.py:101-155): its modules as Kronecker terms (lokr.py)
        from .lokr import terms_from_lycoris
        lyc = terms_from_lycoris(net, cfg, allow_dora=allow_dora)
        terms += [t for t in lyc if not isinstance(t, DoraTerm)]
        dora += [t for t in lyc if isinstance(t, DoraTerm)]
    n_kron = len(terms)
    for mname, mod in decoder.named_modules():
        if hasattr(mod, "modules_to_save") and hasattr(mod, "original_module"):
            raise UnsupportedAdapter(f"modules_to_save wrapper at {mname}: not merged natively")
        if not (hasattr(mod, "lora_A") and hasattr(mod, "lora_B") and hasattr(mod, "scaling")):
            continue
        if getattr(mod, "disable_adapters", False):
            continue
        if getattr(mod, "merged", False) or getattr(mod, "merged_adapters", None):
            raise UnsupportedAdapter(f"PEFT module {mname} has its adapters merged into the weight already")
        if getattr(mod, "fan_in_fan_out", False):
            raise UnsupportedAdapter(f"fan_in_fan_out LoRA at {mname}: not merged natively")
        live = [a for a in _active(mod) if a in mod.lora_A]
        for a in live:
            flag, g = bool((getattr(mod, "use_dora", None) or {}).get(a)), _magnitude(mod, a)
            if (flag or g is not None) and not allow_dora:
                raise UnsupportedAdapter(f"DoRA adapter '{a}' at {mname}: not merged natively")
            if flag != (g is not None):
                raise UnsupportedAdapter(f"adapter '{a}' at {mname}: use_dora and lora_magnitude_vector belong together: not merged natively")
            if flag and len(live) > 1:
                raise UnsupportedAdapter(f"DoRA adapter '{a}' at {mname} beside {len(live) - 1} more active adapter(s): not merged natively")
            if (getattr(mod, "lora_bias", None) or {}).get(a) or getattr(mod.lora_B[a], "bias", None) is not None:
                raise UnsupportedAdapter(f"adapter '{a}' at {mname} trains a bias: not merged natively")
            name = _target_name(_module_path(mname), getattr(cfg, "num_hidden_layers", None))
            terms.append(LoraTerm(name, mod.lora_A[a].weight, mod.lora_B[a].weight, float(mod.scaling[a])))
            if flag:
                dora.append(DoraTerm(name, g.detach(), False, 0.0, 1.0))
                check_g(dora[-1], int(mod.lora_B[a].weight.shape[0]), int(mod.lora_A[a].weight.shape[1]))
    _check_shapes(terms[n_kron:], cfg)
    return terms + dora


def fingerprint(terms) -> tuple:
    """A cheap key of a term list: names, scales, the A / B (for a ``KronTerm``: the factor) storages and their in-place version
    counters; for a ``DoraTerm`` its name, axis, eps, scale and the storage and version of ``g``."""
    def ident(x):
        return None if x is None else (x.data_ptr(), x._version, tuple(x.shape), str(x.device))
    key = []
    for t in terms:
        if hasattr(t, "per_input"):   # ace355.dora.DoraTerm
            key.append(("dora", t.name, bool(t.per_input), float(t.eps), float(t.scale), ident(t.g)))
            continue
        if hasattr(t, "w1_a"):   # ace355.lokr.KronTerm
            key.append(("kron", t.name, float(t.scale)) + tuple(ident(x) for x in t[1:7]))
            continue
        key.append((t.name, float(t.scale), t.A.data_ptr(), t.A._version, tuple(t.A.shape), t.B.data_ptr(), t.B._version,
                    tuple(t.B.shape), str(t.A.device)))
    return tuple(key)
