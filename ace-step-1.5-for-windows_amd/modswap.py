"""NativeModuleSwap: how a native implementation takes the place of a CHILD ``nn.Module`` of the reference model.

``model.encoder`` / ``model.detokenizer`` are registered sub-modules of ``AceStepConditionGenerationModel``
(modeling_acestep_v15_base.py:1571-1573).  ``nn.Module.__setattr__`` refuses to assign a non-Module to such a name, and the
call sites (``prepare_condition``, base.py:1626-1633, 1646-1647; handler/audio_codes.py:49-66) sit OUTSIDE the diffusion seam's
try block (handler/service_generate_execute.py:123), so nothing would catch a native failure there.  This wrapper is an
``nn.Module`` (assignable), keeps the module it replaces as a registered sub-module (state_dict keys unchanged), and delegates to it whenever the native call raises - the same
"try native -> log -> PyTorch" policy as the DiT / VAE seams (handler/service_generate_execute.py:189-191, handler/vae_decode.py:44-48).
"""
from __future__ import annotations

import logging

import torch

logger = logging.getLogger("ace355")


class NativeModuleSwap(torch.nn.Module):
    """Callable like the reference module; ``native_impl`` first, the kept reference module on ValueError / RuntimeError /
    NotImplementedError (unsupported mask form, missing library, failed HIP call)."""

    def __init__(self, native_impl, reference_module: torch.nn.Module, name: str = "module"):
        super().__init__()
        object.__setattr__(self, "_native", native_impl)
        # The kept module is a REAL sub-module (``parent.to()`` / ``half()`` / ``parameters()`` / ``load_state_dict()`` all recurse
        # through the registry: a fallback kept outside it would stay on the old device and miss reloaded weights - exactly when
        # it is needed).  Two hooks keep the parent's state_dict keys the reference's own (no ``_reference.`` segment).
        self._reference = reference_module
        self._swap_name = name
        self.native_calls = 0
        self.native_failures = 0
        self._register_state_dict_hook(self._strip_reference_prefix)
        self._register_load_state_dict_pre_hook(self._add_reference_prefix)
        self.register_load_state_dict_post_hook(self._reload_native)

    @staticmethod
    def _strip_reference_prefix(module, state_dict, prefix, local_metadata):
        inner = prefix + "_reference."
        for k in [k for k in state_dict if k.startswith(inner)]:
            state_dict[prefix + k[len(inner):]] = state_dict.pop(k)
        return state_dict

    @staticmethod
    def _add_reference_prefix(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        inner = prefix + "_reference."
        for k in [k for k in state_dict if k.startswith(prefix) and not k.startswith(inner)]:
            state_dict[inner + k[len(prefix):]] = state_dict.pop(k)

    @staticmethod
    def _reload_native(module, incompatible_keys):
        # weights changed under the wrapper (parent.load_state_dict): the native copy is re-packed from the kept module
        native = native_of(module)
        if hasattr(native, "load_state_dict"):
            try:
                native.load_state_dict(module._reference.state_dict())
            except Exception as exc:  # keep serving through the PyTorch module
                logger.warning("[native-%s] re-packing after load_state_dict failed (%s: %s)", module._swap_name, type(exc).__name__, exc)

    def forward(self, *args, **kwargs):
        try:
            out = self._native(*args, **kwargs)
            self.native_calls += 1
            return out
        except (ValueError, RuntimeError, NotImplementedError) as exc:
            self.native_failures += 1
            if self.native_failures <= 3:
                logger.warning("[native-%s] %s: %s; running the PyTorch module for this call", self._swap_name, type(exc).__name__, exc)
            return self._reference(*args, **kwargs)

    def __getattr__(self, item):
        # attributes of the module it stands in for (config, layers, dtype helpers ...)
        try:
            return super().__getattr__(item)
        except AttributeError:
            if item == "_reference":
                raise
            return getattr(super().__getattr__("_reference"), item)


def native_of(module):
    """The native implementation behind a ``NativeModuleSwap``; any other object is returned as it is."""
    return object.__getattribute__(module, "_native") if isinstance(module, NativeModuleSwap) else module


class _NativeEmbedTokens:
    """``wrapper.embed_tokens``: callable like the reference's ``nn.Embedding``; the native gather first, the kept module's own
    ``embed_tokens`` on ValueError / RuntimeError / NotImplementedError.  Other attributes (``weight``, ``num_embeddings`` ...) are the
    reference embedding's."""

    def __init__(self, swap: "NativeTextEncoderSwap"):
        self._swap = swap

    def __call__(self, ids):
        swap = self._swap
        try:
            out = native_of(swap).embed_tokens(ids)
            swap.native_calls += 1
            return out
        except (ValueError, RuntimeError, NotImplementedError) as exc:
            swap.native_failures += 1
            if swap.native_failures <= 3:
                logger.warning("[native-%s] embed_tokens %s: %s; running the PyTorch embedding for this call", swap._swap_name,
                               type(exc).__name__, exc)
            return swap._reference.embed_tokens(ids)

    def __getattr__(self, item):
        return getattr(self._swap._reference.embed_tokens, item)


class NativeTextEncoderSwap(NativeModuleSwap):
    """``NativeModuleSwap`` for the caption text encoder (``handler.text_encoder``, a ``Qwen3Model``): besides the forward,
    ``embed_tokens`` (conditioning_embed.py:76-79) reaches the native gather - the base class's ``__getattr__`` would hand out the
    reference's ``nn.Embedding`` - with that embedding as the fallback."""

    @property
    def embed_tokens(self):
        return _NativeEmbedTokens(self)


def swap_in_text_encoder(parent, device, attr: str = "text_encoder") -> NativeTextEncoderSwap:
    """``parent.<attr> = NativeTextEncoderSwap(NativeTextEncoder.from_reference(parent.<attr>), parent.<attr>)``; output in the
    module's own dtype.  Raises whatever ``from_reference`` raises (the caller logs and keeps the PyTorch module)."""
    from .textenc import NativeTextEncoder
    ref = getattr(parent, attr)
    if isinstance(ref, NativeModuleSwap):  # re-entry
        ref = ref._reference
    wrapper = NativeTextEncoderSwap(NativeTextEncoder.from_reference(ref, device), ref, attr)
    setattr(parent, attr, wrapper)
    return wrapper


class NativeCausalLMSwap(NativeModuleSwap):
    """``NativeModuleSwap`` for the 5 Hz LM (``LLMHandler.llm``, a ``Qwen3ForCausalLM``), whose forward carries state from call to call.
    The dispatch is on ``past_key_values``: none -> native prefill; the native LM's own token -> native decode; anything else (a cache
    the kept module returned) -> the kept module.  A prefill the native LM refuses (ValueError / RuntimeError / NotImplementedError) runs
    on the kept module, which returns its own cache, so the steps that follow route to it by themselves.  An error inside a native decode
    step propagates: there is no PyTorch cache to continue from.  ``generate``, ``config``, ``generation_config``, ``device`` and every
    other attribute are the kept module's (base class ``__getattr__``), so the non-CFG ``generate()`` path is unchanged."""

    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, **kwargs):
        from .lm import KvToken
        if past_key_values is not None and not isinstance(past_key_values, KvToken):
            return self._reference(input_ids=input_ids, attention_mask=attention_mask, past_key_values=past_key_values, **kwargs)
        if past_key_values is not None:
            out = self._native(input_ids=input_ids, attention_mask=attention_mask, past_key_values=past_key_values, **kwargs)
            self.native_calls += 1
            return out
        try:
            out = self._native(input_ids=input_ids, attention_mask=attention_mask, **kwargs)
            self.native_calls += 1
            return out
        except (ValueError, RuntimeError, NotImplementedError) as exc:
            self.native_failures += 1
            if self.native_failures <= 3:
                logger.warning("[native-%s] %s: %s; running this generation on the PyTorch module", self._swap_name, type(exc).__name__, exc)
            return self._reference(input_ids=input_ids, attention_mask=attention_mask, **kwargs)


def swap_in_lm(parent, device, attr: str = "llm", max_positions: int = 8192, allow_gqa4: bool = False) -> NativeCausalLMSwap:
    """``parent.<attr> = NativeCausalLMSwap(NativeCausalLM.from_reference(parent.<attr>), parent.<attr>)``; logits in the module's own
    dtype.  ``allow_gqa4``: also take Qwen3-4B's 32 / 8 head layout (``NativeCausalLM``).  Raises whatever ``from_reference`` raises
    (the caller logs and keeps the PyTorch module)."""
    from .lm import NativeCausalLM
    ref = getattr(parent, attr)
    if isinstance(ref, NativeModuleSwap):  # re-entry
        ref = ref._reference
    wrapper = NativeCausalLMSwap(NativeCausalLM.from_reference(ref, device, max_positions=max_positions, allow_gqa4=allow_gqa4), ref, attr)
    setattr(parent, attr, wrapper)
    return wrapper


def swap_in(parent: torch.nn.Module, attr: str, native_cls, device, out_dtype: torch.dtype = torch.float32) -> NativeModuleSwap:
    """``parent.<attr> = NativeModuleSwap(native_cls.from_reference(parent.<attr>), parent.<attr>)``; returns the wrapper.
    Raises whatever ``from_reference`` raises (caller logs and keeps the PyTorch module, like ``_init_native_dit``)."""
    ref = getattr(parent, attr)
    if isinstance(ref, NativeModuleSwap):  # re-entry (initialize_service may be called again)
        ref = ref._reference
    wrapper = NativeModuleSwap(native_cls.from_reference(ref, device, out_dtype), ref, attr)
    setattr(parent, attr, wrapper)
    return wrapper
