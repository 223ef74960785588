"""CPU: LoRA adapters on the native DiT - the PEFT reader, the decoder walker, the seam's sync logic, the handler's refusals and the
ABI struct (no GPU, no native compute)."""
import ctypes
import json
import math
import os
import subprocess
import types

import pytest
import torch

import ace355
from ace355 import lora
from ace355.backend import NativeDitMixin, NativeHandler
from ace355.lora import LoraTerm, UnsupportedAdapter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)


def _cfg():
    return ace355.DitConfig(**TINY)


def _write_peft(path, modules, r=4, alpha=8.0, infix=None, fmt="safetensors", extra_cfg=None, metadata=None, seed=0, ranks=None):
    """A PEFT LoRA directory with seeded A / B for `modules` (module paths such as 'layers.0.self_attn.q_proj')."""
    shapes = _cfg().weight_shapes()
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m in modules:
        rr = (ranks or {}).get(m, r)
        out_f, in_f = shapes.get(m + ".weight", (64, 64))
        mid = f".{infix}" if infix else ""
        sd[f"base_model.model.{m}.lora_A{mid}.weight"] = torch.randn(rr, in_f, generator=g)
        sd[f"base_model.model.{m}.lora_B{mid}.weight"] = torch.randn(out_f, rr, generator=g)
    cfg = {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "target_modules": ["q_proj", "k_proj", "v_proj", "o_proj"]}
    cfg.update(extra_cfg or {})
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, os.path.join(path, "adapter_model.safetensors"), metadata=metadata)
    else:
        torch.save(sd, os.path.join(path, "adapter_model.bin"))
    return sd


def test_peft_reader_key_forms_and_scaling(tmp_path):
    mods = ["layers.0.self_attn.q_proj", "layers.1.cross_attn.v_proj", "layers.1.mlp.down_proj"]
    sd = _write_peft(tmp_path / "a", mods, r=4, alpha=8.0)
    terms = {t.name: t for t in lora.read_peft_adapter(str(tmp_path / "a"), _cfg())}
    assert set(terms) == {m + ".weight" for m in mods}
    assert all(t.scale == 2.0 for t in terms.values())   # alpha / r
    assert torch.equal(terms["layers.0.self_attn.q_proj.weight"].A, sd["base_model.model.layers.0.self_attn.q_proj.lora_A.weight"])
    # the in-memory form with the adapter-name infix, and .bin through torch.load(weights_only=True)
    _write_peft(tmp_path / "b", mods, r=4, alpha=8.0, infix="default", fmt="bin")
    tb = {t.name: t for t in lora.read_peft_adapter(str(tmp_path / "b"), _cfg())}
    assert set(tb) == set(terms) and all(torch.equal(tb[k].B, terms[k].B) for k in tb)
    # rsLoRA: alpha / sqrt(r)
    _write_peft(tmp_path / "c", mods, r=4, alpha=8.0, extra_cfg={"use_rslora": True})
    assert all(abs(t.scale - 8.0 / math.sqrt(4)) < 1e-12 for t in lora.read_peft_adapter(str(tmp_path / "c"), _cfg()))
    # rank_pattern / alpha_pattern: matched at a dot boundary at the end of the module name
    _write_peft(tmp_path / "d", mods, r=4, alpha=8.0, ranks={"layers.1.mlp.down_proj": 16},
                extra_cfg={"rank_pattern": {"mlp.down_proj": 16}, "alpha_pattern": {"cross_attn.v_proj": 32, "p_proj": 1000}})
    td = {t.name: t for t in lora.read_peft_adapter(str(tmp_path / "d"), _cfg())}
    assert td["layers.1.mlp.down_proj.weight"].scale == 8.0 / 16
    assert td["layers.1.cross_attn.v_proj.weight"].scale == 32.0 / 4
    assert td["layers.0.self_attn.q_proj.weight"].scale == 8.0 / 4   # ("p_proj" is not a dot-boundary suffix of q_proj)


@pytest.mark.parametrize("case", ["lokr_file", "lokr_meta", "dora", "bias", "lora_bias", "modules_to_save", "fan_in_fan_out", "target",
                                  "loha"])
def test_peft_reader_refuses_what_the_merge_does_not_cover(tmp_path, case):
    p = tmp_path / case
    mods = ["layers.0.self_attn.q_proj"]
    extra, meta = {}, None
    if case == "target":
        mods = ["time_embed.linear_1"]
    elif case == "dora":
        extra = {"use_dora": True}
    elif case == "bias":
        extra = {"bias": "lora_only"}
    elif case == "lora_bias":
        extra = {"lora_bias": True}
    elif case == "modules_to_save":
        extra = {"modules_to_save": ["proj_out"]}
    elif case == "fan_in_fan_out":
        extra = {"fan_in_fan_out": True}
    elif case == "loha":
        extra = {"peft_type": "LOHA"}
    elif case == "lokr_meta":
        meta = {"lokr_config": "{}"}
    _write_peft(p, mods, extra_cfg=extra, metadata=meta)
    if case == "lokr_file":
        (p / "lokr_weights.safetensors").write_bytes(b"")
    with pytest.raises(UnsupportedAdapter):
        lora.read_peft_adapter(str(p), _cfg())


def test_peft_reader_checks_shapes_against_the_config(tmp_path):
    _write_peft(tmp_path / "a", ["layers.0.self_attn.q_proj"])
    small = ace355.DitConfig(hidden_size=128, intermediate_size=768, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1)
    with pytest.raises(ValueError, match="do not fit"):
        lora.read_peft_adapter(str(tmp_path / "a"), small)
    _write_peft(tmp_path / "b", ["layers.5.self_attn.q_proj"])
    with pytest.raises(UnsupportedAdapter):   # layer outside the configuration
        lora.read_peft_adapter(str(tmp_path / "b"), _cfg())


# ---------------------------------------------------------------- decoder walker (PEFT's attributes, no peft import)
class _Lin(torch.nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(o, i))
        self.bias = None


class _LoraLinear(torch.nn.Module):
    def __init__(self, i, o, adapters, r=4):
        super().__init__()
        self.lora_A = torch.nn.ModuleDict({a: _Lin(i, r) for a in adapters})
        self.lora_B = torch.nn.ModuleDict({a: _Lin(r, o) for a in adapters})
        self.scaling = {a: 2.0 for a in adapters}
        self.active_adapters = list(adapters)
        self.disable_adapters = False
        self.merged_adapters = []
        self.use_dora = {a: False for a in adapters}


def _decoder(adapters=("a",)):
    root = torch.nn.Module()
    inner = torch.nn.Module()
    root.base_model = torch.nn.Module()
    root.base_model.model = inner
    inner.layers = torch.nn.ModuleList([torch.nn.Module()])
    inner.layers[0].self_attn = torch.nn.Module()
    inner.layers[0].self_attn.q_proj = _LoraLinear(256, 256, adapters)
    inner.layers[0].mlp = torch.nn.Module()
    inner.layers[0].mlp.up_proj = _LoraLinear(256, 768, adapters)
    return root


def test_decoder_walker():
    dec = _decoder(("a", "b"))
    terms = lora.terms_from_decoder(dec, _cfg())
    assert sorted((t.name, t.scale) for t in terms) == sorted([(n, 2.0) for n in ("layers.0.self_attn.q_proj.weight",
                                                                                   "layers.0.mlp.up_proj.weight") for _ in "ab"])
    q = dec.base_model.model.layers[0].self_attn.q_proj
    assert any(t.A is q.lora_A["b"].weight for t in terms)
    key = lora.fingerprint(terms)
    q.scaling["a"] = 0.5
    assert lora.fingerprint(lora.terms_from_decoder(dec, _cfg())) != key
    for m in (q, dec.base_model.model.layers[0].mlp.up_proj):
        m.disable_adapters = True
    assert lora.terms_from_decoder(dec, _cfg()) == []
    q.disable_adapters = False
    q.merged_adapters = ["a"]
    with pytest.raises(UnsupportedAdapter, match="merged"):
        lora.terms_from_decoder(dec, _cfg())
    q.merged_adapters = []
    q.use_dora["a"] = True
    with pytest.raises(UnsupportedAdapter, match="DoRA"):
        lora.terms_from_decoder(dec, _cfg())
    q.use_dora["a"] = False
    dec._lycoris_net = object()
    with pytest.raises(UnsupportedAdapter, match="LoKr"):
        lora.terms_from_decoder(dec, _cfg())


# ---------------------------------------------------------------- the seam's sync logic
class _RecDit:
    def __init__(self):
        self.calls = []
        self.cfg = _cfg()

    def set_adapters(self, terms):
        self.calls.append(("set", [(t.name, t.scale) for t in terms]))

    def clear_adapters(self):
        self.calls.append(("clear",))


class _Host(NativeDitMixin):
    def __init__(self, decoder=None):
        self.device, self.dtype = "cpu", torch.float32
        self.model = types.SimpleNamespace(null_condition_emb=torch.zeros(1, 1, 8), decoder=decoder or _decoder())
        self.native_dit = _RecDit()
        self.use_lora = False


def _args(B=2, T=6, L=3, D=8):
    return dict(encoder_hidden_states=torch.zeros(B, L, D), encoder_attention_mask=None, context_latents=torch.zeros(B, T, 128),
                src_latents=torch.zeros(B, T, 64), seed=[1, 2])


def test_sync_native_adapters(monkeypatch):
    from ace355 import dit as a_dit
    monkeypatch.setattr(a_dit, "generate_latents", lambda native, null, enc, ctx, **kw: {
        "target_latents": torch.zeros(enc.shape[0], ctx.shape[1], 64), "time_costs": {}})
    h = _Host()
    h._native_run_diffusion(**_args())
    assert h.native_dit.calls == []   # use_lora off, nothing applied: no call
    h.use_lora = True
    h._native_run_diffusion(**_args())
    h._native_run_diffusion(**_args())
    assert [c[0] for c in h.native_dit.calls] == ["set"]   # one merge, then nothing while the fingerprint holds
    h.model.decoder.base_model.model.layers[0].self_attn.q_proj.scaling["a"] = 0.25   # (the reference's set_lora_scale writes scaling)
    h._native_run_diffusion(**_args())
    assert [c[0] for c in h.native_dit.calls] == ["set", "set"] and ("layers.0.self_attn.q_proj.weight", 0.25) in h.native_dit.calls[1][1]
    h.use_lora = False
    h._native_run_diffusion(**_args())
    h._native_run_diffusion(**_args())
    assert [c[0] for c in h.native_dit.calls] == ["set", "set", "clear"]
    h.use_lora = True
    h.model.decoder._lycoris_net = object()
    with pytest.raises(UnsupportedAdapter):   # LoKr: the seam's except runs the PyTorch path
        h._native_run_diffusion(**_args())


def test_sync_is_a_strict_no_op_without_lora():
    class _Host2(NativeDitMixin):
        pass
    h = _Host2()
    h.native_dit = object()   # (no attribute may be read off it)
    h._sync_native_adapters()


# ---------------------------------------------------------------- NativeHandler without a GPU
def test_handler_lora_before_initialize_service_and_data_parallel(tmp_path):
    h = NativeHandler()
    assert h.add_lora(str(tmp_path)) == "❌ Model not initialized. Please initialize service first."
    assert h.load_lora(str(tmp_path)) == "❌ Model not initialized. Please initialize service first."
    assert h.remove_lora("x") == "⚠️ No LoRA adapter loaded."
    assert h.unload_lora() == "⚠️ No LoRA adapter loaded."
    assert h.set_use_lora(True) == "❌ No LoRA adapter loaded. Please load a LoRA first."
    assert h.set_lora_scale(0.5) == "⚠️ No LoRA loaded"
    assert h.set_active_lora_adapter("x") == "❌ Unknown adapter: x"
    # a registry without a native backend (use_native=False): the adapter loads, a data-parallel request with it is refused
    cfg = _cfg()
    from ace355 import weightgen
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=1, mode="test")
    msg, ok = h.initialize_service(cfg, w, torch.zeros(1, 1, 256), device="cpu", use_native=False)
    assert not ok
    _write_peft(tmp_path / "style", ["layers.0.self_attn.q_proj"])
    assert h.add_lora(str(tmp_path / "style")).startswith("✅ LoRA 'style' loaded")
    assert h.add_lora(str(tmp_path / "style")).startswith("❌ Adapter name already in use")
    assert h.set_lora_scale(3.0) == "✅ LoRA scale (style): 1.00"   # clamped to [0, 1]
    assert h.get_lora_status()["active_adapter"] == "style"
    res = h.generate_music(torch.zeros(1, 3, 256), torch.zeros(1, 4, 128), seed=[1], data_parallel=True)
    assert res["success"] is False and "rank-local" in res["error"]
    assert h.set_use_lora(False) == "✅ LoRA disabled"
    assert h.remove_lora("style") == "✅ LoRA unloaded, using base model" and not h.lora_loaded


def test_lora_term_struct_matches_header(tmp_path):
    from ace355 import native
    ct = native.LoraTermC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_lora_term));']
    for fname, _t in ct._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(ace355_lora_term, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 32
    for fname, _t in ct._fields_:
        assert int(got[fname]) == getattr(ct, fname).offset, fname
    assert "ace355_dit_set_adapters" in native.SIGNATURES and "ace355_dit_read_weight" in native.SIGNATURES
