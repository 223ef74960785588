"""CPU: DoRA (weight-decomposed LoRA / LoKr) - the readers with ``allow_dora`` (files and duck-typed modules), the fingerprint, the
seam's sync with a ``DoraTerm``, the handler's scale rule, the DoraTermC layout against the header, and the proof of the exactness gate
the GPU tests apply (tests/_dora_cases.py): an fp32 emulation of the contract passes it on every GPU case's inputs, seeded defects each
fail it."""
import ctypes
import os
import subprocess
import types

import pytest
import torch

import ace355
import _dora_cases as D
import _lokr_cases as L
from ace355 import lokr, lora
from ace355.backend import NativeDitMixin, NativeHandler
from ace355.dora import DoraTerm
from ace355.lora import UnsupportedAdapter
from test_lokr_cpu import _Lokr, _Net, _mod, _tensors, _write
from test_lora_cpu import _decoder, _write_peft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, UP = "layers.0.self_attn.q_proj", "layers.1.mlp.up_proj"


def _cfg():
    return ace355.DitConfig(**D.TINY)


# ---------------------------------------------------------------- the LoKr file reader
def _lokr_file(tmp_path, name, dora_shapes, config, drop=()):
    sd = {**_tensors(Q, 256, 256, r2=4), **_tensors(UP, 768, 256, out_l=24, r2=3)}
    for path, shape in dora_shapes.items():
        if path not in drop:
            sd[_mod(path) + ".dora_scale"] = torch.rand(*shape) + 0.5
    _write(tmp_path / name / "lokr_weights.safetensors", sd, config)
    return sd, str(tmp_path / name)


def test_lokr_file_round_trip_axis_and_eps(tmp_path):
    config = {"linear_dim": 4, "linear_alpha": 2, "weight_decompose": True}
    sd, p = _lokr_file(tmp_path, "a", {Q: (256, 1), UP: (1, 256)}, config)
    with pytest.raises(UnsupportedAdapter, match="DoRA"):   # the default still refuses
        lokr.read_lokr_adapter(p, _cfg())
    terms = lokr.read_lokr_adapter(p, _cfg(), allow_dora=True)
    assert [type(t).__name__ for t in terms] == ["KronTerm", "KronTerm", "DoraTerm", "DoraTerm"]
    d = {t.name: t for t in terms if isinstance(t, DoraTerm)}
    q, up = d[Q + ".weight"], d[UP + ".weight"]
    assert (q.per_input, up.per_input) == (False, True) and q.scale == up.scale == 1.0
    assert q.eps == up.eps == 2.0 ** -7 and q.g.dtype == torch.bfloat16   # the dtype the reference casts its decoder to
    assert torch.equal(q.g, sd[_mod(Q) + ".dora_scale"].to(torch.bfloat16)) and up.g.numel() == 256
    t32 = [t for t in lokr.read_lokr_adapter(p, _cfg(), allow_dora=True, dtype=torch.float32) if isinstance(t, DoraTerm)]
    assert t32[0].eps == 2.0 ** -23 and t32[0].g.dtype == torch.float32 and torch.equal(t32[0].g, sd[_mod(Q) + ".dora_scale"])
    # the additive terms are what the plain reader gives for the same factors
    _write(tmp_path / "plain" / "lokr_weights.safetensors", {k: v for k, v in sd.items() if not k.endswith("dora_scale")},
           {"linear_dim": 4, "linear_alpha": 2})
    plain = lokr.read_lokr_adapter(str(tmp_path / "plain"), _cfg())
    assert [(t.name, t.scale) for t in plain] == [(t.name, t.scale) for t in terms[:2]] and torch.equal(plain[0].w1, terms[0].w1)


def test_lokr_file_refusals(tmp_path):
    on, off = {"linear_dim": 4, "linear_alpha": 2, "weight_decompose": True}, {"linear_dim": 4, "linear_alpha": 2}
    _, p = _lokr_file(tmp_path, "missing", {Q: (256, 1), UP: (1, 256)}, on, drop=(UP,))
    with pytest.raises(UnsupportedAdapter, match="belong together"):   # the metadata without a module's tensor
        lokr.read_lokr_adapter(p, _cfg(), allow_dora=True)
    _, p = _lokr_file(tmp_path, "nometa", {Q: (256, 1), UP: (1, 256)}, off)
    with pytest.raises(UnsupportedAdapter, match="belong together"):   # the tensors without the metadata
        lokr.read_lokr_adapter(p, _cfg(), allow_dora=True)
    with pytest.raises(UnsupportedAdapter, match="DoRA"):
        lokr.read_lokr_adapter(p, _cfg())
    for shape in ((256,), (256, 256), (1, 768), (2, 128)):
        _, p = _lokr_file(tmp_path, "shape" + "x".join(map(str, shape)), {Q: shape, UP: (768, 1)}, on)
        with pytest.raises(ValueError, match="neither"):
            lokr.read_lokr_adapter(p, _cfg(), allow_dora=True)
    sd, p = _lokr_file(tmp_path, "tucker", {Q: (256, 1), UP: (1, 256)}, dict(on, use_tucker=True))
    with pytest.raises(UnsupportedAdapter, match="tucker"):
        lokr.read_lokr_adapter(p, _cfg(), allow_dora=True)
    sd[_mod(Q) + ".lokr_t2"] = torch.randn(4, 4, 1, 1)
    _write(tmp_path / "t2" / "lokr_weights.safetensors", sd, on)
    with pytest.raises(UnsupportedAdapter, match="Tucker"):
        lokr.read_lokr_adapter(str(tmp_path / "t2"), _cfg(), allow_dora=True)
    sd = {**_tensors(Q, 256, 256, r2=4), _mod("time_embed.linear_1") + ".dora_scale": torch.ones(256, 1)}
    _write(tmp_path / "foreign" / "lokr_weights.safetensors", sd, on)
    with pytest.raises(UnsupportedAdapter, match="outside"):
        lokr.read_lokr_adapter(str(tmp_path / "foreign"), _cfg(), allow_dora=True)


# ---------------------------------------------------------------- the live LyCORIS form
def _wd_decoder():
    a, b = _Lokr(Q, 256, 256), _Lokr(UP, 768, 256, out_l=24, r2=3)
    for mod, shape in ((a, (256, 1)), (b, (1, 256))):
        mod.wd, mod.bypass_mode = True, False
        mod.dora_scale = torch.nn.Parameter((torch.rand(*shape) + 0.5).to(torch.bfloat16))
    dec = torch.nn.Module()
    dec._lycoris_net = _Net([a, b])
    return dec


def test_live_lycoris_form():
    dec = _wd_decoder()
    net = dec._lycoris_net
    with pytest.raises(UnsupportedAdapter, match="LoKr.*DoRA"):
        lora.terms_from_decoder(dec, _cfg())
    terms = lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    assert [type(t).__name__ for t in terms] == ["KronTerm", "KronTerm", "DoraTerm", "DoraTerm"]
    q, up = terms[2], terms[3]
    assert (q.name, q.per_input, q.eps, q.scale) == (Q + ".weight", False, 2.0 ** -7, 1.0) and up.per_input is True
    assert q.g.data_ptr() == net.loras[0].dora_scale.data_ptr()
    net.set_multiplier(0.5)   # m enters the Kronecker scale and the interpolation
    t = lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    assert (t[0].scale, t[2].scale) == (0.25, 0.5)
    net.loras[0].dora_scale = torch.nn.Parameter(torch.ones(256, 1))   # eps follows the dtype of dora_scale
    assert lora.terms_from_decoder(dec, _cfg(), allow_dora=True)[2].eps == 2.0 ** -23
    net.loras[0].bypass_mode = True
    with pytest.raises(UnsupportedAdapter, match="bypass_mode"):
        lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    net.loras[0].bypass_mode = False
    net.loras[0].dora_scale = None
    with pytest.raises(UnsupportedAdapter, match="belong together"):
        lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    net.loras[0].dora_scale = torch.nn.Parameter(torch.ones(256))
    with pytest.raises(ValueError, match="neither"):
        lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    net.loras[0].dora_scale = torch.nn.Parameter(torch.ones(256, 1))
    net.loras[0].lokr_t2 = torch.nn.Parameter(torch.randn(4, 4, 1, 1))
    with pytest.raises(UnsupportedAdapter, match="Tucker"):
        lora.terms_from_decoder(dec, _cfg(), allow_dora=True)


# ---------------------------------------------------------------- PEFT use_dora, both forms
@pytest.mark.parametrize("form", ["parameter", "module", "infix"])
def test_peft_file_round_trip(tmp_path, form):
    mods = [Q, "layers.1.mlp.down_proj"]
    sd = _write_peft(tmp_path / "a", mods, extra_cfg={"use_dora": True})
    g = {m: torch.rand(_cfg().weight_shapes()[m + ".weight"][0]) + 0.5 for m in mods}
    key = {"parameter": "{}.lora_magnitude_vector", "module": "{}.lora_magnitude_vector.weight",
           "infix": "{}.lora_magnitude_vector.default.weight"}[form]
    for m in mods:
        sd[key.format("base_model.model." + m)] = g[m]
    from safetensors.torch import save_file
    save_file(sd, str(tmp_path / "a" / "adapter_model.safetensors"))
    with pytest.raises(UnsupportedAdapter, match="DoRA"):
        lora.read_peft_adapter(str(tmp_path / "a"), _cfg())
    terms = lora.read_peft_adapter(str(tmp_path / "a"), _cfg(), allow_dora=True)
    assert [type(t).__name__ for t in terms] == ["LoraTerm", "LoraTerm", "DoraTerm", "DoraTerm"]
    for t in terms[2:]:
        assert (t.per_input, t.eps, t.scale) == (False, 0.0, 1.0) and torch.equal(t.g, g[t.name[:-len(".weight")]])
    assert {t.scale for t in terms[:2]} == {2.0}


def test_peft_file_refusals(tmp_path):
    from safetensors.torch import save_file
    sd = _write_peft(tmp_path / "flag", [Q], extra_cfg={"use_dora": True})   # the flag without a vector
    with pytest.raises(UnsupportedAdapter, match="belong together"):
        lora.read_peft_adapter(str(tmp_path / "flag"), _cfg(), allow_dora=True)
    sd = _write_peft(tmp_path / "vec", [Q])                                   # a vector without the flag
    sd[f"base_model.model.{Q}.lora_magnitude_vector"] = torch.ones(256)
    save_file(sd, str(tmp_path / "vec" / "adapter_model.safetensors"))
    with pytest.raises(UnsupportedAdapter, match="belong together"):
        lora.read_peft_adapter(str(tmp_path / "vec"), _cfg(), allow_dora=True)
    with pytest.raises(UnsupportedAdapter, match="DoRA"):
        lora.read_peft_adapter(str(tmp_path / "vec"), _cfg())
    sd = _write_peft(tmp_path / "orphan", [Q], extra_cfg={"use_dora": True})  # DoRA keys for a target without an A / B pair
    sd[f"base_model.model.{Q}.lora_magnitude_vector"] = torch.ones(256)
    sd["base_model.model.layers.1.self_attn.k_proj.lora_magnitude_vector"] = torch.ones(128)
    save_file(sd, str(tmp_path / "orphan" / "adapter_model.safetensors"))
    with pytest.raises(UnsupportedAdapter, match="no lora_A / lora_B pair"):
        lora.read_peft_adapter(str(tmp_path / "orphan"), _cfg(), allow_dora=True)
    sd = _write_peft(tmp_path / "len", [Q], extra_cfg={"use_dora": True})
    sd[f"base_model.model.{Q}.lora_magnitude_vector"] = torch.ones(255)
    save_file(sd, str(tmp_path / "len" / "adapter_model.safetensors"))
    with pytest.raises(ValueError, match="does not hold"):
        lora.read_peft_adapter(str(tmp_path / "len"), _cfg(), allow_dora=True)


class _Mag(torch.nn.Module):   # newer PEFT: a DoraLinearLayer with a .weight
    def __init__(self, n):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.rand(n) + 0.5)


@pytest.mark.parametrize("form", ["parameter", "module"])
def test_live_peft_form(form):
    dec = _decoder(("a",))
    q = dec.base_model.model.layers[0].self_attn.q_proj
    q.use_dora["a"] = True
    q.lora_magnitude_vector = torch.nn.ParameterDict({"a": torch.nn.Parameter(torch.rand(256) + 0.5)}) if form == "parameter" \
        else torch.nn.ModuleDict({"a": _Mag(256)})
    held = q.lora_magnitude_vector["a"] if form == "parameter" else q.lora_magnitude_vector["a"].weight
    with pytest.raises(UnsupportedAdapter, match="DoRA"):
        lora.terms_from_decoder(dec, _cfg())
    terms = lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    assert [type(t).__name__ for t in terms] == ["LoraTerm", "LoraTerm", "DoraTerm"]
    d = terms[2]
    assert (d.name, d.per_input, d.eps, d.scale) == (Q + ".weight", False, 0.0, 1.0) and d.g.data_ptr() == held.data_ptr()
    q.scaling["a"] = 0.5   # the user's scale changes s only
    t = lora.terms_from_decoder(dec, _cfg(), allow_dora=True)
    assert t[0].scale == 0.5 and t[2].scale == 1.0
    two = _decoder(("a", "b"))
    q2 = two.base_model.model.layers[0].self_attn.q_proj
    q2.use_dora["a"] = True
    q2.lora_magnitude_vector = torch.nn.ParameterDict({"a": torch.nn.Parameter(torch.ones(256))})
    with pytest.raises(UnsupportedAdapter, match="more active adapter"):
        lora.terms_from_decoder(two, _cfg(), allow_dora=True)
    q.use_dora["a"] = False   # a vector without the flag
    with pytest.raises(UnsupportedAdapter, match="belong together"):
        lora.terms_from_decoder(dec, _cfg(), allow_dora=True)


# ---------------------------------------------------------------- fingerprint
def test_fingerprint_of_a_dora_term():
    g = torch.ones(256)
    t = DoraTerm(Q + ".weight", g, False, 2.0 ** -7, 1.0)
    key = lora.fingerprint([t])
    assert key == (("dora", Q + ".weight", False, 2.0 ** -7, 1.0, (g.data_ptr(), g._version, (256,), "cpu")),)
    assert lora.fingerprint([t]) == key
    assert lora.fingerprint([t._replace(scale=0.6)]) != key and lora.fingerprint([t._replace(per_input=True)]) != key
    assert lora.fingerprint([t._replace(eps=0.0)]) != key
    g.mul_(2.0)   # in place
    assert lora.fingerprint([t]) != key
    dec = _wd_decoder()
    k0 = lora.fingerprint(lora.terms_from_decoder(dec, _cfg(), allow_dora=True))
    with torch.no_grad():
        dec._lycoris_net.loras[1].dora_scale.add_(1.0)
    assert lora.fingerprint(lora.terms_from_decoder(dec, _cfg(), allow_dora=True)) != k0


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
        self.model = types.SimpleNamespace(null_condition_emb=torch.zeros(1, 1, 8), decoder=_wd_decoder())
        self.native_dit = _RecDit()
        self.use_lora = False


def test_sync_native_adapters_with_dora_modules():
    h = _Host()
    h._sync_native_adapters()
    assert h.native_dit.calls == []
    h.use_lora = True
    h._sync_native_adapters()   # (the seam asks with allow_dora=True: no UnsupportedAdapter)
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set"]
    assert h.native_dit.calls[0][1] == [("KronTerm", Q + ".weight", 0.5), ("KronTerm", UP + ".weight", 0.5),
                                        ("DoraTerm", Q + ".weight", 1.0), ("DoraTerm", UP + ".weight", 1.0)]
    h.model.decoder._lycoris_net.set_multiplier(0.5)
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set", "set"] and [x[2] for x in h.native_dit.calls[1][1]] == [0.25, 0.25, 0.5, 0.5]
    with torch.no_grad():
        h.model.decoder._lycoris_net.loras[0].dora_scale.mul_(1.5)   # a trained magnitude changes in place: one more merge
    h._sync_native_adapters()
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set", "set", "set"]
    h.use_lora = False
    h._sync_native_adapters()
    assert [c[0] for c in h.native_dit.calls] == ["set", "set", "set", "clear"]


def test_handler_scale_rule(tmp_path):
    """The user's scale multiplies a DoraTerm's m for a LoKr adapter (LyCORIS' multiplier) and not for a PEFT one."""
    from ace355 import weightgen
    from safetensors.torch import save_file
    cfg = _cfg()
    h = NativeHandler()
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=1, mode="test")
    _, ok = h.initialize_service(cfg, w, torch.zeros(1, 1, 256), device="cpu", use_native=False)
    assert not ok
    _, p = _lokr_file(tmp_path, "style", {Q: (256, 1), UP: (1, 256)}, {"linear_dim": 4, "linear_alpha": 2, "weight_decompose": True})
    assert h.add_lora(p) == f"✅ LoRA 'style' loaded from {p}" and h._adapter_type == "lokr"
    terms = h._native_adapter_terms()
    assert [(type(t).__name__, t.scale) for t in terms] == [("KronTerm", 0.5), ("KronTerm", 0.5), ("DoraTerm", 1.0), ("DoraTerm", 1.0)]
    assert all(t.g.dtype == torch.float32 and t.g.dim() == 1 and t.eps == 2.0 ** -23 for t in terms[2:])   # (this handler's dtype: fp32)
    assert h.set_lora_scale(0.5) == "✅ LoKr scale (style): 0.50"
    assert [t.scale for t in h._native_adapter_terms()] == [0.25, 0.25, 0.5, 0.5]
    assert h.unload_lora() == "✅ LoRA unloaded, using base model"
    sd = _write_peft(tmp_path / "peft", [Q], extra_cfg={"use_dora": True})
    sd[f"base_model.model.{Q}.lora_magnitude_vector"] = torch.rand(256) + 0.5
    save_file(sd, str(tmp_path / "peft" / "adapter_model.safetensors"))
    assert h.add_lora(str(tmp_path / "peft")).startswith("✅ LoRA 'peft' loaded") and h._adapter_type == "lora"
    assert h.set_lora_scale(0.5) == "✅ LoRA scale (peft): 0.50"
    assert [(type(t).__name__, t.scale) for t in h._native_adapter_terms()] == [("LoraTerm", 1.0), ("DoraTerm", 1.0)]
    _, p = _lokr_file(tmp_path, "tucker", {Q: (256, 1), UP: (1, 256)}, {"use_tucker": True, "weight_decompose": True})
    h.unload_lora()
    assert h.add_lora(p).startswith("❌ Failed to load LoRA: LoKr adapter with use_tucker") and not h.lora_loaded


# ---------------------------------------------------------------- the C ABI mirror
def test_dora_term_struct_matches_header(tmp_path):
    from ace355 import native
    ct = native.DoraTermC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_dora_term));']
    for fname, _t in ct._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(ace355_dora_term, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 32
    for fname, _t in ct._fields_:
        assert int(got[fname]) == getattr(ct, fname).offset, fname
    assert "ace355_dit_set_adapters_dora" in native.SIGNATURES
    assert hasattr(native.lib(), "ace355_dit_set_adapters_dora")
    assert len(DoraTerm._fields) == 5 and DoraTerm._fields == ("name", "g", "per_input", "eps", "scale")


# ---------------------------------------------------------------- the proof of the gate
@pytest.fixture(scope="module")
def tiny():
    from ace355 import weightgen
    cfg = _cfg()
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=11, mode="test")   # (what test_lora_gpu._make loads)
    return cfg, w, D.tiny_cases(cfg, w)


def test_fp32_emulation_passes_the_gate_on_every_gpu_case(tiny):
    cfg, w, cases = tiny
    n, worst_near = 0, 0.0
    for label, terms in cases:
        add, dr = D.split_terms(terms)
        for name, d in dr.items():
            w0 = w[name].to(torch.bfloat16)
            same, near, worst = D.gate(D.emulate(w0, add[name], d), w0, add[name], d, (label, name))
            assert same >= 0.999
            worst_near = max(worst_near, near)
            n += 1
    assert n >= 80 and worst_near <= 0.01   # (the shares sit well under the 2 % cap: the cap does not decide these cases)
    labels = " ".join(l for l, _ in cases)
    for word in ("axis in", "axis out", "m 1.0", "m 0.6", "eps 0.0", f"eps {D.EPS_BF16}", "lora", "full", "all ten kinds", "some targets"):
        assert word in labels, word


def _cases_for(defect, cases):
    """The cases on which a defect shows at all."""
    for label, terms in cases:
        if not label[0] in "(fl":   # the per-kind cases: a LoKr split, "full", "lora"
            continue
        add, dr = D.split_terms(terms)
        for name, d in dr.items():
            if defect == "drop_eps" and d.eps == 0.0 or defect == "drop_m" and d.scale == 1.0:
                continue
            if defect == "g_by_packed_row" and (d.per_input or not any(k in name for k in D.HEADPAIR_KINDS + D.IL32_KINDS)):
                continue
            yield label, name, add[name], d


@pytest.mark.parametrize("defect", [x for x in D.DEFECTS if x != "fp32_accumulation"])
def test_seeded_defects_fail_the_gate(tiny, defect):
    cfg, w, cases = tiny
    n = 0
    for label, name, ts, d in _cases_for(defect, cases):
        w0 = w[name].to(torch.bfloat16)
        with pytest.raises(AssertionError):
            D.gate(D.emulate(w0, ts, d, defect), w0, ts, d, (defect, label, name))
        n += 1
    assert n >= 6, n


def test_fp32_accumulation_fails_the_gate_at_6144_columns():
    """The reason for fp64: a sequential fp32 sum of 6144 squares leaves the norm further from the exact one than E allows, and
    the gate sees it; the contract's fp64 sum passes on the same inputs."""
    g = torch.Generator().manual_seed(3000)
    name, shape = "layers.0.mlp.down_proj.weight", (256, 6144)
    w0 = (torch.randn(shape, generator=g) * 0.02).to(torch.bfloat16)
    ts = [L.make_term(name, shape, (16, 64, 0, 0), g, w0=w0.float())]
    d = D.make_dora(name, w0, ts, False, 1.0, D.EPS_BF16, g)
    D.gate(D.emulate(w0, ts, d), w0, ts, d, "fp64 accumulation, 256 x 6144", tie_cap=0.05)
    with pytest.raises(AssertionError):
        D.gate(D.emulate(w0, ts, d, "fp32_accumulation"), w0, ts, d, "fp32 accumulation, 256 x 6144", tie_cap=0.05)
