"""LoKr (LyCORIS Kronecker) adapters for the native DiT: read them from disk or from a decoder's LyCORIS network as merge terms.

The reference's promoted adapter family: it trains LoKr through LyCORIS (acestep/training/lokr_utils.py, configs.py:42-75), loads
``lokr_weights.safetensors`` with ``create_lycoris`` + ``load_weights`` (core/generation/handler/lora/lifecycle.py:16-155, 232-236) and
toggles / scales it with ``set_multiplier`` (controls.py:12-32, 49-55, 121-129).  A LoKr module on a Linear ``[out, in]`` adds
``scale * multiplier * scalar * kron(W1, W2)`` to the weight, ``W1 [out_l, in_m]`` and ``W2 [out_k, in_n]`` each held in full
(``lokr_w1``) or as a product (``lokr_w1_a @ lokr_w1_b``).  The native handle merges exactly that into its packed bf16 weights
(``NativeDit.set_adapters``, include/ace355.h ``ace355_dit_set_adapters_mixed``).

The LyCORIS conventions used here - the ``lycoris_<path with underscores>`` module names, the attribute and state-dict names, the scale
rules (``alpha / dim``, ``alpha / sqrt(dim)`` with rs_lora, 1 for a module whose two factors are both full) - are restated from its
published ``LokrModule``; ``lycoris`` is neither imported here nor part of the reference tree, so they are unpinned.  What the merge
does not cover raises ``UnsupportedAdapter``: Tucker (``lokr_t2``), other LyCORIS algorithms, and targets outside the ten projection
kinds.  DoRA (``weight_decompose`` / ``dora_scale``, on by default in the reference's training API) is merged too, but it is not an
additive term: the readers return it as ``ace355.dora.DoraTerm`` only to a caller that asks with ``allow_dora=True`` and refuse it
otherwise, so that a caller that sums ``dense_delta`` is never silently wrong.
"""
from __future__ import annotations

import json
import logging
import math
import os
from typing import Dict, List, NamedTuple, Optional

import torch

from .dora import DoraTerm, axis_of, dora_eps
from .lora import LOKR_WEIGHTS_FILENAME, TARGET_KINDS, UnsupportedAdapter

logger = logging.getLogger(__name__)

# LoKRConfig defaults (acestep/training/configs.py:42-58)
LOKR_CONFIG_DEFAULTS = dict(linear_dim=64, linear_alpha=128, factor=-1, decompose_both=False, use_tucker=False, use_scalar=False,
                            weight_decompose=False, target_modules=["q_proj", "k_proj", "v_proj", "o_proj"], full_matrix=False,
                            bypass_mode=False, rs_lora=False, unbalanced_factorization=False)
_SUFFIXES = ("lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b", "alpha", "scalar")


class KronTerm(NamedTuple):
    name: str                        # reference key of the target weight
    w1: Optional[torch.Tensor]       # [out_l, in_m], or None with w1_a [out_l, r1] and w1_b [r1, in_m]
    w1_a: Optional[torch.Tensor]
    w1_b: Optional[torch.Tensor]
    w2: Optional[torch.Tensor]       # [out_k, in_n], or None with w2_a [out_k, r2] and w2_b [r2, in_n]
    w2_a: Optional[torch.Tensor]
    w2_b: Optional[torch.Tensor]
    scale: float                     # LyCORIS scale x multiplier x scalar (x the user's scale where the caller applies one)


def lycoris_names(num_layers: int) -> Dict[str, str]:
    """``lora_name`` of every target module -> reference key of its weight (LyCORIS: prefix + '_' + module path, dots as underscores)."""
    return {"lycoris_" + f"layers.{i}.{kind}".replace(".", "_"): f"layers.{i}.{kind}.weight"
            for i in range(num_layers) for kind in TARGET_KINDS}


def term_dims(t: KronTerm):
    """(out_l, out_k, in_m, in_n, r1, r2) of a term; ValueError where the factor tensors do not fit one another."""
    def one(w, a, b, which):
        if (w is None) == (a is None and b is None) or (a is None) != (b is None):
            raise ValueError(f"LoKr term {t.name}: give {which} or {which}_a and {which}_b")
        if w is not None:
            if w.dim() != 2:
                raise ValueError(f"LoKr term {t.name}: {which} {tuple(w.shape)} is not a matrix")
            return int(w.shape[0]), int(w.shape[1]), 0
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0] or a.shape[1] < 1:
            raise ValueError(f"LoKr term {t.name}: {which}_a {tuple(a.shape)} / {which}_b {tuple(b.shape)} do not multiply")
        return int(a.shape[0]), int(b.shape[1]), int(a.shape[1])
    out_l, in_m, r1 = one(t.w1, t.w1_a, t.w1_b, "w1")
    out_k, in_n, r2 = one(t.w2, t.w2_a, t.w2_b, "w2")
    return out_l, out_k, in_m, in_n, r1, r2


def check_shapes(terms: List[KronTerm], cfg) -> None:
    if cfg is None:
        return
    shapes = cfg.weight_shapes()
    for t in terms:
        out_f, in_f = shapes[t.name]
        out_l, out_k, in_m, in_n, _, _ = term_dims(t)
        if out_l * out_k != out_f or in_m * in_n != in_f:
            raise ValueError(f"LoKr shapes for {t.name}: W1 [{out_l}, {in_m}] kron W2 [{out_k}, {in_n}] do not fit the weight "
                             f"[{out_f}, {in_f}] of this configuration")


def dense_delta(t: KronTerm, dtype=torch.float64) -> torch.Tensor:
    """``scale * kron(W1, W2)`` of a term in ``dtype`` from the factors as held (tests, export)."""
    w1 = t.w1.to(dtype) if t.w1 is not None else t.w1_a.to(dtype) @ t.w1_b.to(dtype)
    w2 = t.w2.to(dtype) if t.w2 is not None else t.w2_a.to(dtype) @ t.w2_b.to(dtype)
    return t.scale * torch.kron(w1, w2)


# ---------------------------------------------------------------- the file path
def is_lokr_safetensors(path: str) -> bool:
    """lifecycle.py:16-35: the LoKr artefact name, or any safetensors file with a non-empty ``lokr_config`` metadata string."""
    if not os.path.isfile(path) or not path.lower().endswith(".safetensors"):
        return False
    if os.path.basename(path) == LOKR_WEIGHTS_FILENAME:
        return True
    try:
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as sf:
            meta = sf.metadata() or {}
    except Exception:
        return False
    raw = meta.get("lokr_config")
    return isinstance(raw, str) and bool(raw.strip())


def resolve_lokr_weights_path(adapter_path: str) -> Optional[str]:
    """lifecycle.py:38-57: a LoKr file itself, ``lokr_weights.safetensors`` in a directory, or a file there with the metadata."""
    if os.path.isfile(adapter_path):
        return adapter_path if is_lokr_safetensors(adapter_path) else None
    if os.path.isdir(adapter_path):
        p = os.path.join(adapter_path, LOKR_WEIGHTS_FILENAME)
        if os.path.exists(p):
            return p
        try:
            entries = sorted(os.listdir(adapter_path))
        except OSError:
            return None
        for name in entries:
            cand = os.path.join(adapter_path, name)
            if is_lokr_safetensors(cand):
                return cand
    return None


def load_lokr_config(weights_path: str) -> dict:
    """lifecycle.py:60-98: the ``lokr_config`` metadata over the ``LoKRConfig`` defaults; unknown keys are dropped, a missing or
    invalid value keeps the default."""
    cfg = dict(LOKR_CONFIG_DEFAULTS)
    try:
        from safetensors import safe_open
        with safe_open(weights_path, framework="pt", device="cpu") as sf:
            meta = sf.metadata() or {}
    except Exception as exc:
        logger.warning("Unable to read LoKr metadata from %s: %s", weights_path, exc)
        return cfg
    raw = meta.get("lokr_config")
    if not isinstance(raw, str) or not raw.strip():
        return cfg
    try:
        parsed = json.loads(raw)
    except json.JSONDecodeError as exc:
        logger.warning("Invalid LoKr metadata config JSON in %s: %s", weights_path, exc)
        return cfg
    if not isinstance(parsed, dict):
        return cfg
    for k, v in parsed.items():
        if k not in cfg:
            continue
        d = cfg[k]
        if isinstance(d, bool):
            ok = isinstance(v, bool)
        elif isinstance(d, int):
            ok = isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and (k != "linear_dim" or v >= 1)
        else:
            ok = isinstance(v, list)
        if ok:
            cfg[k] = v
        else:
            logger.warning("LoKr metadata %s=%r in %s is invalid; keeping the default %r", k, v, weights_path, d)
    return cfg


def lokr_scale(cfg: dict, both_full: bool) -> float:
    """The module scale LyCORIS sets at creation (the reference creates the modules from the metadata, ``load_weights`` only fills
    tensors): ``alpha / dim``, ``alpha / sqrt(dim)`` with rs_lora, and 1 for a module whose two factors are both full matrices."""
    if both_full:
        return 1.0
    dim, alpha = float(cfg["linear_dim"]), float(cfg["linear_alpha"])
    return alpha / (math.sqrt(dim) if cfg["rs_lora"] else dim)


def read_lokr_adapter(path: str, cfg=None, allow_dora: bool = False, dtype: torch.dtype = torch.bfloat16) -> list:
    """Terms (CPU tensors) of the LoKr artefact ``path`` (a directory or a file, resolved as the reference resolves it).  ``cfg`` (a
    ``DitConfig``) checks every target's shape.  A weight-decomposed adapter (``weight_decompose`` metadata with a ``dora_scale``
    tensor per module; one without the other is refused) needs ``allow_dora=True`` and adds one ``DoraTerm`` per module behind the
    ``KronTerm`` list: the axis from the tensor's shape, the magnitudes cast to ``dtype`` and ``eps = finfo(dtype).eps``, ``dtype``
    being what the reference casts its decoder to."""
    wp = resolve_lokr_weights_path(path)
    if wp is None:
        raise ValueError(f"expected a LoKr artefact ({LOKR_WEIGHTS_FILENAME}, or a safetensors file with lokr_config metadata): {path}")
    from safetensors.torch import load_file
    lc = load_lokr_config(wp)
    if lc["weight_decompose"] and not allow_dora:
        raise UnsupportedAdapter("LoKr adapter with weight_decompose (DoRA): not merged natively")
    if lc["use_tucker"]:
        raise UnsupportedAdapter("LoKr adapter with use_tucker: not merged natively")
    sd = load_file(wp)
    num_layers = getattr(cfg, "num_hidden_layers", None)
    names = lycoris_names(num_layers if num_layers is not None else 100)
    parts: Dict[str, Dict[str, torch.Tensor]] = {}
    for key, t in sd.items():
        mod, _, suffix = key.rpartition(".")
        if suffix == "lokr_t2":
            raise UnsupportedAdapter(f"LoKr tensor '{key}' (Tucker): not merged natively")
        if suffix == "dora_scale" and not allow_dora:
            raise UnsupportedAdapter(f"LoKr tensor '{key}' (DoRA): not merged natively")
        if (suffix not in _SUFFIXES and suffix != "dora_scale") or not mod:
            raise UnsupportedAdapter(f"LoKr adapter tensor '{key}' is not a LoKr factor, alpha or scalar")
        if mod not in names:
            raise UnsupportedAdapter(f"LoKr target '{mod}' is outside the projections the native DiT merges "
                                     "(lycoris_layers_{i}_{self_attn,cross_attn}_{q,k,v,o}_proj, lycoris_layers_{i}_mlp_{gate,up,down}_proj)")
        parts.setdefault(mod, {})[suffix] = t
    terms, dora = [], []
    for mod, p in parts.items():
        if ("dora_scale" in p) != bool(lc["weight_decompose"]):
            raise UnsupportedAdapter(f"LoKr module {mod}: weight_decompose metadata and a dora_scale tensor belong together; "
                                     f"{'the tensor is missing' if lc['weight_decompose'] else 'the metadata does not set it'}")
        f = {s: p.get("lokr_" + s) for s in ("w1", "w1_a", "w1_b", "w2", "w2_a", "w2_b")}
        t = KronTerm(names[mod], f["w1"], f["w1_a"], f["w1_b"], f["w2"], f["w2_a"], f["w2_b"], 1.0)
        try:
            term_dims(t)
        except ValueError as exc:
            raise ValueError(f"LoKr module {mod}: {exc}") from None
        scale = lokr_scale(lc, t.w1 is not None and t.w2 is not None)
        if "alpha" in p and float(p["alpha"].float().reshape(-1)[0]) / float(lc["linear_dim"]) != scale:
            logger.warning("LoKr module %s: stored alpha %g contradicts the scale %g the lokr_config metadata gives; the metadata holds "
                           "(the reference creates its modules from it)", mod, float(p["alpha"].float().reshape(-1)[0]), scale)
        if "scalar" in p:
            scale *= float(p["scalar"].float().reshape(-1)[0])
        terms.append(t._replace(scale=scale))
        if "dora_scale" in p:
            out_l, out_k, in_m, in_n, _, _ = term_dims(t)
            ds = p["dora_scale"]
            dora.append(DoraTerm(t.name, ds.to(dtype), axis_of(ds.shape, out_l * out_k, in_m * in_n, f"LoKr module {mod}"),
                                 dora_eps(dtype), 1.0))
    check_shapes(terms, cfg)
    return terms + dora


# ---------------------------------------------------------------- the live path
def _num(x) -> float:
    return float(x.detach().float().reshape(-1)[0]) if isinstance(x, torch.Tensor) else float(x)


def terms_from_lycoris(net, cfg=None, allow_dora: bool = False) -> list:
    """Terms of a decoder's ``_lycoris_net``, by duck typing (no ``lycoris`` import): every module of ``net.loras`` is read as a
    LokrModule - ``lora_name``, ``lokr_w1`` or ``lokr_w1_a`` / ``lokr_w1_b``, ``lokr_w2`` or ``lokr_w2_a`` / ``lokr_w2_b``, and the
    term scale ``scale x multiplier x scalar`` (``set_multiplier``, the reference's toggle and scale control, writes ``multiplier``).
    ``bypass_mode`` computes the same linear map and is accepted.  A module with ``wd`` and a ``dora_scale`` needs
    ``allow_dora=True`` and adds a ``DoraTerm`` behind the ``KronTerm`` list: ``g`` the ``dora_scale`` tensor itself, ``eps`` of its
    dtype, ``scale = multiplier``.  Weight decomposition happens in the module's forward and not in bypass: both set is refused."""
    loras = getattr(net, "loras", None)
    if loras is None or isinstance(loras, (str, bytes)) or not hasattr(loras, "__iter__"):
        raise UnsupportedAdapter("LoKr / LyCORIS network on the decoder without a readable `loras` list: not merged natively")
    num_layers = getattr(cfg, "num_hidden_layers", None)
    names = lycoris_names(num_layers if num_layers is not None else 100)
    terms, dora = [], []
    for mod in loras:
        lname = getattr(mod, "lora_name", None)
        if getattr(mod, "lokr_t2", None) is not None or getattr(mod, "tucker", False):
            raise UnsupportedAdapter(f"LoKr module {lname} uses Tucker decomposition (lokr_t2): not merged natively")
        wd, ds = bool(getattr(mod, "wd", False)), getattr(mod, "dora_scale", None)
        if (wd or ds is not None) and not allow_dora:
            raise UnsupportedAdapter(f"LoKr module {lname} uses weight decomposition (DoRA): not merged natively")
        if wd != (ds is not None):
            raise UnsupportedAdapter(f"LoKr module {lname}: wd and dora_scale belong together: not merged natively")
        if wd and getattr(mod, "bypass_mode", False):
            raise UnsupportedAdapter(f"LoKr module {lname} sets both wd (DoRA) and bypass_mode: not merged natively")
        f = {s: getattr(mod, "lokr_" + s, None) for s in ("w1", "w1_a", "w1_b", "w2", "w2_a", "w2_b")}
        if not isinstance(lname, str) or (f["w1"] is None and f["w1_a"] is None) or (f["w2"] is None and f["w2_a"] is None):
            raise UnsupportedAdapter(f"LyCORIS module {lname or type(mod).__name__} is not a LoKr module: not merged natively")
        if lname not in names:
            raise UnsupportedAdapter(f"LoKr target '{lname}' is outside the projections the native DiT merges")
        scale = _num(getattr(mod, "scale", 1.0)) * _num(getattr(mod, "multiplier", 1.0)) * _num(getattr(mod, "scalar", 1.0))
        t = KronTerm(names[lname], f["w1"], f["w1_a"], f["w1_b"], f["w2"], f["w2_a"], f["w2_b"], scale)
        out_l, out_k, in_m, in_n, _, _ = term_dims(t)
        terms.append(t)
        if wd:
            dora.append(DoraTerm(t.name, ds.detach(), axis_of(ds.shape, out_l * out_k, in_m * in_n, f"LoKr module {lname}"),
                                 dora_eps(ds.dtype), _num(getattr(mod, "multiplier", 1.0))))
    check_shapes(terms, cfg)
    return terms + dora
