"""CPU: the LoKr readers (lokr_weights.safetensors files and a duck-typed LyCORIS network), the seam's sync with Kronecker terms, the
handler's messages and state, the KronTermC layout against the header, and the proof of the exactness gate the GPU tests apply
(tests/_lokr_cases.py): an fp32 emulation of the contract passes it on every GPU case's inputs, seeded defects each fail it."""
import ctypes
import json
import logging
import os
import subprocess
import types

import pytest
import torch
from safetensors.torch import save_file

import ace355
import _lokr_cases as L
from ace355 import lokr, lora
from ace355.backend import NativeDitMixin, NativeHandler
from ace355.lora import UnsupportedAdapter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return ace355.DitConfig(**L.TINY)


def _mod(path):
    return "lycoris_" + path.replace(".", "_")


def _tensors(path, out_f, in_f, out_l=16, in_m=16, r1=0, r2=0, alpha=None, scalar=None):
    m, sd = _mod(path), {}
    out_k, in_n = out_f // out_l, in_f // in_m
    if r1:
        sd[f"{m}.lokr_w1_a"], sd[f"{m}.lokr_w1_b"] = torch.randn(out_l, r1), torch.randn(r1, in_m)
    else:
        sd[f"{m}.lokr_w1"] = torch.randn(out_l, in_m)
    if r2:
        sd[f"{m}.lokr_w2_a"], sd[f"{m}.lokr_w2_b"] = torch.randn(out_k, r2), torch.randn(r2, in_n)
    else:
        sd[f"{m}.lokr_w2"] = torch.randn(out_k, in_n)
    if alpha is not None:
        sd[f"{m}.alpha"] = torch.tensor(float(alpha))
    if scalar is not None:
        sd[f"{m}.scalar"] = torch.tensor(float(scalar))
    return sd


def _write(file, sd, config=None, raw_meta=None):
    os.makedirs(os.path.dirname(str(file)), exist_ok=True)
    meta = raw_meta if raw_meta is not None else ({"lokr_config": json.dumps(config)} if config is not None else None)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(file), metadata=meta)


# ---------------------------------------------------------------- the file reader
def test_reader_resolves_directory_bare_file_and_custom_name(tmp_path):
    sd = {**_tensors("layers.0.self_attn.q_proj", 256, 256, r2=4), **_tensors("layers.1.mlp.down_proj", 256, 768, out_l=8, in_m=24)}
    _write(tmp_path / "d" / "lokr_weights.safetensors", sd, {"linear_dim": 4, "linear_alpha": 2})
    for p in (tmp_path / "d", tmp_path / "d" / "lokr_weights.safetensors"):
        terms = {t.name: t for t in lokr.read_lokr_adapter(str(p), _cfg())}
        assert set(terms) == {"layers.0.self_attn.q_proj.weight", "layers.1.mlp.down_proj.weight"}
        q, d = terms["layers.0.self_attn.q_proj.weight"], terms["layers.1.mlp.down_proj.weight"]
        assert q.w2 is None and q.w2_a.shape == (16, 4) and q.w1.shape == (16, 16) and q.scale == 0.5
        assert d.w1.shape == (8, 24) and d.w2.shape == (32, 32) and d.scale == 1.0   # both factors full: scale 1
        assert lokr.term_dims(q) == (16, 16, 16, 16, 0, 4) and lokr.term_dims(d) == (8, 32, 24, 32, 0, 0)
    # a custom file name is a LoKr artefact through its metadata only
    _write(tmp_path / "c" / "my_adapter.safetensors", sd, {"linear_dim": 4, "linear_alpha": 4})
    assert lokr.resolve_lokr_weights_path(str(tmp_path / "c")) == str(tmp_path / "c" / "my_adapter.safetensors")
    assert {t.scale for t in lokr.read_lokr_adapter(str(tmp_path / "c"), _cfg())} == {1.0}
    assert lokr.read_lokr_adapter(str(tmp_path / "c" / "my_adapter.safetensors"), _cfg())
    _write(tmp_path / "n" / "other.safetensors", sd)   # no metadata, not the artefact name: not LoKr
    assert lokr.resolve_lokr_weights_path(str(tmp_path / "n")) is None and lokr.resolve_lokr_weights_path(str(tmp_path / "n" / "other.safetensors")) is None
    with pytest.raises(ValueError, match="expected a LoKr artefact"):
        lokr.read_lokr_adapter(str(tmp_path / "n"), _cfg())
    # the dense delta of a term is scale x kron(W1, W2)
    q = [t for t in lokr.read_lokr_adapter(str(tmp_path / "d"), _cfg()) if "q_proj" in t.name][0]
    want = 0.5 * torch.kron(q.w1.double(), q.w2_a.double() @ q.w2_b.double())
    assert torch.equal(lokr.dense_delta(q), want) and want[16 * 3 + 5, 16 * 7 + 2] == 0.5 * q.w1.double()[3, 7] * (q.w2_a.double() @ q.w2_b.double())[5, 2]


def test_reader_scale_rules_and_config_fallbacks(tmp_path, caplog):
    one = lambda **kw: _tensors("layers.0.self_attn.q_proj", 256, 256, **kw)
    read = lambda p: lokr.read_lokr_adapter(str(p), _cfg())[0].scale
    _write(tmp_path / "a" / "lokr_weights.safetensors", one(r2=4))                       # no metadata: LoKRConfig defaults, 128 / 64
    assert read(tmp_path / "a") == 2.0
    _write(tmp_path / "b" / "lokr_weights.safetensors", one(r2=4), {"linear_dim": 16, "linear_alpha": 4, "rs_lora": True})
    assert read(tmp_path / "b") == 1.0                                                   # 4 / sqrt(16)
    _write(tmp_path / "c" / "lokr_weights.safetensors", one(r1=2, r2=4), {"linear_dim": 8, "linear_alpha": 2, "decompose_both": True})
    assert read(tmp_path / "c") == 0.25
    _write(tmp_path / "d" / "lokr_weights.safetensors", one(), {"linear_dim": 8, "linear_alpha": 2})
    assert read(tmp_path / "d") == 1.0                                                   # both full
    _write(tmp_path / "e" / "lokr_weights.safetensors", one(r2=4, scalar=0.5, alpha=2), {"linear_dim": 8, "linear_alpha": 2, "use_scalar": True})
    with caplog.at_level(logging.WARNING, logger="ace355.lokr"):
        caplog.clear()
        assert read(tmp_path / "e") == 0.125 and not caplog.records                     # alpha agrees: no warning
        _write(tmp_path / "f" / "lokr_weights.safetensors", one(r2=4, alpha=8), {"linear_dim": 8, "linear_alpha": 2})
        assert read(tmp_path / "f") == 0.25 and any("contradicts" in r.getMessage() for r in caplog.records)
    # invalid metadata values and invalid JSON fall back to the defaults; unknown keys are dropped
    _write(tmp_path / "g" / "lokr_weights.safetensors", one(r2=4), {"linear_dim": "x", "linear_alpha": 32, "rs_lora": "yes", "nonsense": 1})
    cfgd = lokr.load_lokr_config(str(tmp_path / "g" / "lokr_weights.safetensors"))
    assert cfgd["linear_dim"] == 64 and cfgd["linear_alpha"] == 32 and cfgd["rs_lora"] is False and "nonsense" not in cfgd
    assert read(tmp_path / "g") == 0.5
    _write(tmp_path / "h" / "lokr_weights.safetensors", one(r2=4), raw_meta={"lokr_config": "{not json"})
    assert lokr.load_lokr_config(str(tmp_path / "h" / "lokr_weights.safetensors")) == lokr.LOKR_CONFIG_DEFAULTS and read(tmp_path / "h") == 2.0


@pytest.mark.parametrize("case", ["weight_decompose", "use_tucker", "lokr_t2", "dora_scale", "suffix", "foreign_target", "layer_outside"])
def test_reader_refuses_what_the_merge_does_not_cover(tmp_path, case):
    sd, config = _tensors("layers.0.self_attn.q_proj", 256, 256, r2=4), {"linear_dim": 4, "linear_alpha": 4}
    if case in ("weight_decompose", "use_tucker"):
        config[case] = True
    elif case == "lokr_t2":
        sd[_mod("layers.0.self_attn.q_proj") + ".lokr_t2"] = torch.randn(4, 4, 1, 1)
    elif case == "dora_scale":
        sd[_mod("layers.0.self_attn.q_proj") + ".dora_scale"] = torch.randn(1, 256)
    elif case == "suffix":
        sd[_mod("layers.0.self_attn.q_proj") + ".hada_w1_a"] = torch.randn(4, 4)
    elif case == "foreign_target":
        sd.update(_tensors("time_embed.linear_1", 256, 256))
    elif case == "layer_outside":
        sd.update(_tensors("layers.5.self_attn.q_proj", 256, 256))
    _write(tmp_path / "x" / "lokr_weights.safetensors", sd, config)
    with pytest.raises(UnsupportedAdapter):
        lokr.read_lokr_adapter(str(tmp_path / "x"), _cfg())


def test_reader_checks_shapes(tmp_path):
    _write(tmp_path / "a" / "lokr_weights.safetensors", _tensors("layers.0.self_attn.q_proj", 256, 256, r2=4), {})
    small = ace355.DitConfig(hidden_size=128, intermediate_size=768, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1)
    with pytest.raises(ValueError, match="do not fit"):
        lokr.read_lokr_adapter(str(tmp_path / "a"), small)
    sd = _tensors("layers.0.self_attn.q_proj", 256, 256, r2=4)
    del sd[_mod("layers.0.self_attn.q_proj") + ".lokr_w2_b"]
    _write(tmp_path / "b" / "lokr_weights.safetensors", sd, {})
    with pytest.raises(ValueError, match="w2 or w2_a and w2_b"):
        lokr.read_lokr_adapter(str(tmp_path / "b"), _cfg())
    sd = _tensors("layers.0.self_attn.q_proj", 256, 256, r2=4)
    sd[_mod("layers.0.self_attn.q_proj") + ".lokr_w2_b"] = torch.randn(5, 16)
    _write(tmp_path / "c" / "lokr_weights.safetensors", sd, {})
    with pytest.raises(ValueError, match="do not multiply"):
        lokr.read_lokr_adapter(str(tmp_path / "c"), _cfg())
    sd = _tensors("layers.0.self_attn.q_proj", 256, 256)
    sd[_mod("layers.0.self_attn.q_proj") + ".lokr_w2_a"] = torch.randn(16, 4)   # a full and a decomposed W2
    sd[_mod("layers.0.self_attn.q_proj") + ".lokr_w2_b"] = torch.randn(4, 16)
    _write(tmp_path / "d" / "lokr_weights.safetensors", sd, {})
    with pytest.raises(ValueError, match="w2 or w2_a and w2_b"):
        lokr.read_lokr_adapter(str(tmp_path / "d"), _cfg())


def test_peft_reader_still_refuses_lokr_artefacts(tmp_path):
    _write(tmp_path / "a" / "lokr_weights.safetensors", _tensors("layers.0.self_attn.q_proj", 256, 256), {})
    with pytest.raises(UnsupportedAdapter, match="LoKr"):
        lora.read_peft_adapter(str(tmp_path / "a"), _cfg())


# ---------------------------------------------------------------- the duck-typed reader (LyCORIS' attributes, no lycoris import)
class _Lokr(torch.nn.Module):
    def __init__(self, path, out_f, in_f, out_l=16, in_m=16, r2=4, scale=0.5):
        super().__init__()
        self.lora_name = _mod(path)
        self.lokr_w1 = torch.nn.Parameter(torch.randn(out_l, in_m))
        self.lokr_w2_a = torch.nn.Parameter(torch.randn(out_f // out_l, r2))
        self.lokr_w2_b = torch.nn.Parameter(torch.randn(r2, in_f // in_m))
        self.scale, self.multiplier, self.bypass_mode = scale, 1.0, True
        self.register_buffer("scalar", torch.tensor(1.0))


class _Net(torch.nn.Module):
    def __init__(self, mods):
        super().__init__()
        self.loras = torch.nn.ModuleList(mods)

    def set_multiplier(self, m):   # (LycorisNetwork.set_multiplier)
        for x in self.loras:
            x.multiplier = m


def _lyco_decoder():
    dec = torch.nn.Module()
    dec._lycoris_net = _Net([_Lokr("layers.0.self_attn.q_proj", 256, 256), _Lokr("layers.1.mlp.up_proj", 768, 256, out_l=24, r2=3)])
    return dec


def test_duck_typed_reader():
    dec = _lyco_decoder()
    net = dec._lycoris_net
    terms = lora.terms_from_decoder(dec, _cfg())
    assert [(t.name, t.scale) for t in terms] == [("layers.0.self_attn.q_proj.weight", 0.5), ("layers.1.mlp.up_proj.weight", 0.5)]
    assert terms[0].w1 is net.loras[0].lokr_w1 and terms[0].w2 is None and terms[1].w2_b is net.loras[1].lokr_w2_b
    keys = set()
    for m in (1.0, 0.5, 0.0):   # the reference's toggle and scale controls (controls.py:12-32)
        net.set_multiplier(m)
        t = lora.terms_from_decoder(dec, _cfg())
        assert [x.scale for x in t] == [0.5 * m, 0.5 * m]
        assert lora.fingerprint(t) == lora.fingerprint(lora.terms_from_decoder(dec, _cfg()))
        keys.add(lora.fingerprint(t))
    assert len(keys) == 3
    net.set_multiplier(1.0)
    key = lora.fingerprint(lora.terms_from_decoder(dec, _cfg()))
    with torch.no_grad():
        net.loras[0].lokr_w1.mul_(2.0)   # an in-place update of a factor
    assert lora.fingerprint(lora.terms_from_decoder(dec, _cfg())) != key
    net.loras[0].scalar.fill_(0.25)
    assert lora.terms_from_decoder(dec, _cfg())[0].scale == 0.125
    net.loras[0].scalar.fill_(1.0)
    # refusals
    net.loras[0].lokr_t2 = torch.nn.Parameter(torch.randn(4, 4, 1, 1))
    with pytest.raises(UnsupportedAdapter, match="LoKr.*Tucker"):
        lora.terms_from_decoder(dec, _cfg())
    del net.loras[0].lokr_t2
    net.loras[0].wd = True
    with pytest.raises(UnsupportedAdapter, match="LoKr.*DoRA"):
        lora.terms_from_decoder(dec, _cfg())
    net.loras[0].wd = False
    foreign = torch.nn.Module()
    foreign.lora_name, foreign.hada_w1_a = _mod("layers.0.self_attn.k_proj"), torch.nn.Parameter(torch.randn(4, 4))
    dec._lycoris_net = _Net([foreign])
    with pytest.raises(UnsupportedAdapter, match="not a LoKr module"):
        lora.terms_from_decoder(dec, _cfg())
    dec._lycoris_net = _Net([_Lokr("time_embed.linear_1", 256, 256)])
    with pytest.raises(UnsupportedAdapter, match="LoKr target"):
        lora.terms_from_decoder(dec, _cfg())
    dec._lycoris_net = _Net([_Lokr("layers.0.self_attn.q_proj", 256, 512)])
    with pytest.raises(ValueError, match="do not fit"):
        lora.terms_from_decoder(dec, _cfg())
    plain = torch.nn.Module()
    plain._lycoris_net = object()   # a net without a `loras` list
    with pytest.raises(UnsupportedAdapter, match="LoKr"):
        lora.terms_from_decoder(plain, _cfg())


def test_peft_modules_beside_a_lycoris_net_are_still_read():
    from test_lora_cpu import _decoder
    dec = _decoder()
    dec._lycoris_net = _Net([_Lokr("layers.1.mlp.up_proj", 768, 256, out_l=24)])
    terms = lora.terms_from_decoder(dec, _cfg())
    assert [type(t).__name__ for t in terms] == ["KronTerm", "LoraTerm", "LoraTerm"]
    key = lora.fingerprint(terms)
    assert key[0][0] == "kron" and key[1][0] == "layers.0.self_attn.q_proj.weight"   # LoraTerm keys are what they were


def test_fingerprint_of_lora_terms_is_unchanged():
    A, B = torch.randn(4, 256), torch.randn(256, 4)
    t = lora.LoraTerm("layers.0.self_attn.q_proj.weight", A, B, 0.5)
    assert lora.fingerprint([t]) == (("layers.0.self_attn.q_proj.weight", 0.5, A.data_ptr(), A._version, (4, 256), B.data_ptr(), B._version,
                                      (256, 4), "cpu"),)


# ---------------------------------------------------------------- the seam's sync logic
class _RecDit:
    def __init__(self):
        self.calls = []
        self.cfg = _cfg()

    def set_adapters(self, terms):
        self.calls.append(("set", [(type(t).__name__, t.name, t.scale) for t in terms]))

    def clear_adapters(self):
        self.calls.append(("clear",))


class _Host(NativeDitMixin):
    def __init__(self):
        self.device, self.dtype = "cpu", torch.float32
        self.model = types.SimpleNamespace(null_condition_emb=torch.zeros(1, 1, 8), decoder=_lyco_decoder())
        self.native_dit = _RecDit()
        self.use_lora = False


def test_sync_native_adapters_with_a_lycoris_net():
    h = _Host()
    h._sync_native_adapters()
    assert h.native_dit.calls == []
    h.use_lora = True
    h._sync_native_adapters()
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set"] and h.native_dit.calls[0][1][0] == ("KronTerm", "layers.0.self_attn.q_proj.weight", 0.5)
    h.model.decoder._lycoris_net.set_multiplier(0.5)   # set_lora_scale(0.5) in the reference
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set", "set"] and h.native_dit.calls[1][1][0][2] == 0.25
    h.model.decoder._lycoris_net.set_multiplier(0.0)   # set_use_lora(False) in the reference zeroes the multiplier and clears use_lora
    h.use_lora = False
    h._sync_native_adapters()
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set", "set", "clear"]


# ---------------------------------------------------------------- NativeHandler without a GPU
def test_handler_messages_and_state(tmp_path):
    from ace355 import weightgen
    from test_lora_cpu import _write_peft
    cfg = _cfg()
    h = NativeHandler()
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=1, mode="test")
    msg, ok = h.initialize_service(cfg, w, torch.zeros(1, 1, 256), device="cpu", use_native=False)
    assert not ok
    lk = tmp_path / "style"
    _write(lk / "lokr_weights.safetensors", _tensors("layers.0.self_attn.q_proj", 256, 256, r2=4), {"linear_dim": 4, "linear_alpha": 2})
    assert h.add_lora(str(lk)) == f"✅ LoRA 'style' loaded from {lk}"
    assert h._adapter_type == "lokr" and h.lora_loaded and h.use_lora
    st = h.get_lora_status()
    assert st["adapter_type"] == "lokr" and st["label"] == "LoKr" and st["active_adapter"] == "style"
    terms = h._native_adapter_terms()
    assert [type(t).__name__ for t in terms] == ["KronTerm"] and terms[0].scale == 0.5
    assert h.set_lora_scale(0.5) == "✅ LoKr scale (style): 0.50" and h._native_adapter_terms()[0].scale == 0.25
    assert h.set_use_lora(False) == "✅ LoKr disabled"
    assert h.set_lora_scale(3.0) == "✅ LoKr scale (style): 1.00 (LoKr disabled)"
    assert h.set_use_lora(True) == "✅ LoKr enabled"
    assert h.add_lora(str(lk), "second") == "❌ A LoKr adapter is loaded; unload it before loading another adapter."
    res = h.generate_music(torch.zeros(1, 3, 256), torch.zeros(1, 4, 128), seed=[1], data_parallel=True)
    assert res["success"] is False and "rank-local" in res["error"]
    assert h.remove_lora("style") == "✅ LoRA unloaded, using base model" and h._adapter_type is None and not h.lora_loaded
    assert h.load_lora(str(lk)) == f"✅ LoKr loaded from {lk / 'lokr_weights.safetensors'}"
    assert h.unload_lora() == "✅ LoRA unloaded, using base model" and h._adapter_type is None
    assert h.set_use_lora(True) == "❌ No LoRA adapter loaded. Please load a LoRA first."
    # LoKr as a second adapter behind a PEFT LoRA: the reference's refusal (lifecycle.py:244-246)
    _write_peft(tmp_path / "peft", ["layers.0.self_attn.q_proj"])
    assert h.add_lora(str(tmp_path / "peft")).startswith("✅ LoRA 'peft' loaded") and h._adapter_type == "lora"
    assert h.add_lora(str(lk)) == "❌ LoKr cannot be added as a second adapter when PEFT is already loaded."
    assert h.set_use_lora(False) == "✅ LoRA disabled"
    assert h.unload_lora() == "✅ LoRA unloaded, using base model"
    # a LoKr artefact the merge does not cover is reported, and nothing is loaded
    _write(tmp_path / "tucker" / "lokr_weights.safetensors", _tensors("layers.0.self_attn.q_proj", 256, 256), {"use_tucker": True})
    assert h.add_lora(str(tmp_path / "tucker")).startswith("❌ Failed to load LoRA: LoKr adapter with use_tucker") and not h.lora_loaded


# ---------------------------------------------------------------- the C ABI mirror
def test_kron_term_struct_matches_header(tmp_path):
    from ace355 import native
    ct = native.KronTermC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_kron_term));']
    for fname, _t in ct._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(ace355_kron_term, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 88
    for fname, _t in ct._fields_:
        assert int(got[fname]) == getattr(ct, fname).offset, fname
    assert "ace355_dit_set_adapters_mixed" in native.SIGNATURES
    assert hasattr(native.lib(), "ace355_dit_set_adapters_mixed")


# ---------------------------------------------------------------- the proof of the gate
@pytest.fixture(scope="module")
def tiny():
    from ace355 import weightgen
    cfg = _cfg()
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=11, mode="test")   # (what test_lora_gpu._make loads)
    return cfg, w, L.tiny_cases(cfg, w)


def test_fp32_emulation_passes_the_gate_on_every_gpu_case(tiny):
    cfg, w, cases = tiny
    n = 0
    for label, terms in cases:
        for name, ts in L.by_target(terms).items():
            w0 = w[name].to(torch.bfloat16)
            same, near, worst = L.gate(L.emulate(w0, ts), w0, ts, (label, name))
            assert same >= 0.999
            n += 1
    assert n >= 40


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_seeded_defects_fail_the_gate(tiny, defect):
    cfg, w, cases = tiny
    cases = dict(cases)
    n = 0
    for label in ("split (16, 64, 0, 8)", "split (8, 32, 4, 40)", "two terms on one target, relative size 3"):
        for name, ts in L.by_target(cases[label]).items():
            if defect == "drop_second_term" and len(ts) < 2:
                continue
            if defect == "bf16_w2" and ts[0].w2 is not None:
                continue
            w0 = w[name].to(torch.bfloat16)
            with pytest.raises(AssertionError):
                L.gate(L.emulate(w0, ts, defect), w0, ts, (defect, label, name))
            n += 1
    assert n >= 2
