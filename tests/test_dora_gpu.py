"""GPU: DoRA (weight-decomposed LoRA / LoKr) merged into the packed DiT weights (ace355_dit_set_adapters_dora) - merge exactness
under the derived gate of tests/_dora_cases.py, parity against the oracle on the float64-merged weights under the LoRA tests'
effect-size rule, bit identity across the adapter lifecycle, stale condition slots, every refusal, and the handler end to end from a
weight-decomposed lokr_weights.safetensors file and from a PEFT use_dora directory."""
import json
import os
import time

import pytest
import torch

import _dora_cases as D
import _drift
import _lokr_cases as L
from test_lokr_gpu import _all_bits, _default_lokr_terms, _mixed_call, _names, _same, _write_lokr
from test_lora_gpu import KINDS, TINY, _bits, _effect_rule, _fwd_inputs, _make, _sampler_case, _terms, _twin, _write_peft

pytestmark = pytest.mark.gpu


def _w0(w):
    return {n: t.to(torch.bfloat16) for n, t in w.items() if n.startswith("layers.") and n.endswith("_proj.weight")}


def _with_dora(add, w, seed, per_input=lambda i: i % 2 == 1, m=1.0, eps=D.EPS_BF16):
    """``add`` (one additive term per target) plus a DoraTerm on each target."""
    g = torch.Generator().manual_seed(seed)
    w0 = _w0(w)
    return list(add) + [D.make_dora(t.name, w0[t.name], [t], per_input(i), m, eps, g) for i, t in enumerate(add)]


def test_merge_exactness_tiny(gpu_device):
    cfg, w, dit = _make(gpu_device)
    base = {n: dit.read_weight(n, torch.bfloat16).cpu() for n in _names(cfg)}
    for label, terms in D.tiny_cases(cfg, w):
        add, dora = D.split_terms(terms)
        dit.set_adapters([t for t in terms if not D.is_dora(t)])
        plain = {n: dit.read_weight(n, torch.bfloat16).cpu() for n in add}
        dit.set_adapters(terms)
        assert dit.adapters_applied
        for n in base:
            got = dit.read_weight(n, torch.bfloat16).cpu()
            if n not in add:
                assert torch.equal(_bits(got), _bits(base[n])), f"untouched {n} changed ({label})"
            elif n not in dora:   # a target without a DoRA term keeps the bits of the plain merge
                assert torch.equal(_bits(got), _bits(plain[n])), f"{n} without a DoRA term differs from the plain merge ({label})"
            else:
                D.gate(got, base[n], add[n], dora[n], (label, n))
                differs = float((_bits(got) != _bits(plain[n])).float().mean())
                assert differs >= 0.9, (label, n, "share of elements that differ from the plain additive merge", differs)
    dit.clear_adapters()
    assert not dit.adapters_applied
    for n, b in base.items():
        assert torch.equal(_bits(dit.read_weight(n, torch.bfloat16).cpu()), _bits(b)), n
    dit.close()


def test_merge_full_size_fresh_handle(gpu_device):
    """The real architecture on a FRESH handle: the default LoKr configuration (q / k / v / o of both attentions, 24 layers) with DoRA
    on the output axis, eps 2^-7; the gate on the eight kinds of three layers.  The merge times are printed, not asserted."""
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    from ace355.dora import DoraTerm
    cfg = ace355.DitConfig()
    dit = NativeDit(cfg, gpu_device)
    for name, shape in cfg.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
        native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
    native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
    attn = [k for k in KINDS if "attn" in k]
    add = _default_lokr_terms(cfg, gpu_device, attn)
    assert len(add) == 8 * cfg.num_hidden_layers
    gated = [f"layers.{li}.{k}.weight" for li in (0, 11, 23) for k in attn]
    g = torch.Generator().manual_seed(2)
    w0, dora = {}, []
    for t in add:
        out_f = cfg.weight_shapes()[t.name][0]
        if t.name in gated:   # g around the exact norms, as in the tiny cases
            w0[t.name] = weightgen.make_dit_weights({t.name: cfg.weight_shapes()[t.name]}, cfg.hidden_size, seed=4, mode="test")[t.name] \
                .to(torch.bfloat16).to(gpu_device)
            dora.append(D.make_dora(t.name, w0[t.name], [t], False, 1.0, D.EPS_BF16, g))
        else:
            dora.append(DoraTerm(t.name, (1 + 0.25 * torch.randn(out_f, generator=g)).to(torch.bfloat16), False, D.EPS_BF16, 1.0))
    dora = [d._replace(g=d.g.to(gpu_device, torch.float32)) for d in dora]   # (what the seam holds: the timings exclude the upload)
    ms, ms_plain = [], []
    for terms, out in ((add, ms_plain), (add + dora, ms)):
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dit.set_adapters(terms)
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
    print(f"full size, default LoKr configuration (q/k/v/o of both attentions x 24 layers): plain set_adapters {ms_plain[0]:.2f} ms (first: "
          f"+ pristine copies), then {ms_plain[1]:.2f} / {ms_plain[2]:.2f} ms; with DoRA {ms[0]:.2f} / {ms[1]:.2f} / {ms[2]:.2f} ms")
    by = L.by_target(add)
    dby = {d.name: d for d in dora}
    for name in gated:
        D.gate(dit.read_weight(name, torch.bfloat16), w0[name], by[name], dby[name], name, tie_cap=0.05)
    dit.close()


def test_tiny_forward_with_dora_vs_oracle(gpu_device):
    from oracle import dit as o_dit
    cfg, w, dit = _make(gpu_device)
    terms = _with_dora(L.all_kinds_terms(cfg, w, seed=3, rel_size=1.5), w, seed=5)
    x, ctx, enc, t, tr = _fwd_inputs(cfg)

    def hip():
        for n in range(3):
            dit.set_condition(n, enc[n])
        return dit.forward(x, ctx, t, tr, [0, 1, 2]).cpu()
    hb = hip()
    dit.set_adapters(terms)
    hl = hip()
    oc = o_dit.DitConfig(**TINY)
    args = (x, torch.tensor(t), torch.tensor(tr), enc, ctx)
    wm = D.merged(w, terms)   # the float64 DoRA merge, handed to the oracle as fp32
    ref_b, ref_l = o_dit.dit_forward(oc, w, *args), o_dit.dit_forward(oc, wm, *args)
    emu_b, emu_l = _drift.emulated(o_dit.dit_forward, oc, w, *args), _drift.emulated(o_dit.dit_forward, oc, wm, *args)
    _effect_rule("tiny forward, LoKr + DoRA on ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def test_tiny_sampler_with_dora_vs_oracle(gpu_device):
    from ace355.dit import generate_latents
    from oracle import dit as o_dit, sampler as o_sampler
    cfg, w, dit = _make(gpu_device)
    terms = _with_dora(L.all_kinds_terms(cfg, w, seed=4, rel_size=1.5), w, seed=6)
    null, enc, ctx, kw = _sampler_case(cfg)
    hb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    dit.set_adapters(terms)
    hl = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    oc, wm = o_dit.DitConfig(**TINY), D.merged(w, terms)
    ref_b, ref_l = o_sampler.generate_audio(oc, w, null, enc, ctx, **kw), o_sampler.generate_audio(oc, wm, null, enc, ctx, **kw)
    emu_b = _drift.emulated(o_sampler.generate_audio, oc, w, null, enc, ctx, **kw)
    emu_l = _drift.emulated(o_sampler.generate_audio, oc, wm, null, enc, ctx, **kw)
    _effect_rule("tiny sampler 27 steps CFG 7 + APG, LoKr + DoRA on ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def test_lifecycle_bits(gpu_device):
    """DoRA -> plain LoKr -> DoRA against fresh twins; m 1 -> 0.6 -> 0 (base bits) -> 1; the same call twice; PEFT-style DoRA on LoRA
    terms beside LoKr + DoRA in one call."""
    cfg, w, dit = _make(gpu_device)
    base = _all_bits(dit, cfg)
    lokr = L.all_kinds_terms(cfg, w, seed=21)
    dora = _with_dora(lokr, w, seed=22)

    def scaled(m):   # LyCORIS' multiplier: in the Kronecker scale and in the interpolation
        return [t._replace(scale=t.scale * m) for t in dora]

    def fresh(terms):
        _, _, d = _make(gpu_device)
        d.set_adapters(terms)
        bits = _all_bits(d, cfg)
        d.close()
        return bits
    f_dora, f_lokr, f_06 = fresh(dora), fresh(lokr), fresh(scaled(0.6))
    assert not _same(f_dora, f_lokr) and not _same(f_dora, f_06)
    dit.set_adapters(dora)
    a = _all_bits(dit, cfg)
    dit.set_adapters(dora)
    assert _same(a, _all_bits(dit, cfg)) and _same(a, f_dora) and dit.adapters_applied   # the same call twice: bit-identical
    dit.set_adapters(lokr)
    assert _same(_all_bits(dit, cfg), f_lokr)
    dit.set_adapters(dora)
    assert _same(_all_bits(dit, cfg), f_dora)
    dit.set_adapters(scaled(0.6))
    assert _same(_all_bits(dit, cfg), f_06)
    dit.set_adapters(scaled(0.0))
    assert _same(_all_bits(dit, cfg), base) and not dit.adapters_applied
    dit.set_adapters(scaled(1.0))
    assert _same(_all_bits(dit, cfg), f_dora)
    # a DoRA term at m = 0 beside live additive terms is dropped: the plain merge
    dit.set_adapters([t._replace(scale=0.0) if D.is_dora(t) else t for t in dora])
    assert _same(_all_bits(dit, cfg), f_lokr)
    # both families decomposed in one call, disjoint targets: each target as in the call of its own family
    lora = [t for t in _terms(cfg, w, rank=8, seed=23) if "mlp" in t.name]
    peft = lora + [D.make_dora(t.name, _w0(w)[t.name], [t], False, 1.0, 0.0, torch.Generator().manual_seed(24)) for t in lora]
    f_peft = fresh(peft)
    dit.set_adapters(peft + [t for t in dora if "attn" in t.name])
    m = _all_bits(dit, cfg)
    assert all(torch.equal(m[n], (f_peft if "mlp" in n else f_dora)[n]) for n in m)
    dit.clear_adapters()
    assert _same(_all_bits(dit, cfg), base)
    dit.close()


def _dora_call(dit, lora_terms=(), kron_terms=(), dora_rows=()):
    """ace355_dit_set_adapters_dora through ctypes; dora_rows as DoraTermC rows."""
    from ace355 import native
    from ace355.lokr import term_dims
    keep, rows, krows = [], [], []
    dev = lambda x: None if x is None else x.to(dit.device, torch.bfloat16).contiguous()
    for t in lora_terms:
        a, b = dev(t.A), dev(t.B)
        keep += [a, b]
        rows.append(native.LoraTermC(t.name.encode(), native.ptr(a), native.ptr(b), a.shape[0], float(t.scale)))
    for t in kron_terms:
        f = [dev(x) for x in t[1:7]]
        keep += f
        krows.append(native.KronTermC(t.name.encode(), *[native.ptr(x) if x is not None else 0 for x in f], *term_dims(t), float(t.scale)))
    arr = (native.LoraTermC * max(len(rows), 1))(*rows)
    karr = (native.KronTermC * max(len(krows), 1))(*krows)
    darr = (native.DoraTermC * max(len(dora_rows), 1))(*dora_rows)
    with torch.cuda.device(dit.device):
        return dit._lib.ace355_dit_set_adapters_dora(dit._h, arr, len(rows), karr, len(krows), darr, len(dora_rows),
                                                     native.current_stream_ptr())


def test_dora_call_without_dora_terms_is_set_adapters_mixed(gpu_device):
    cfg, w, dit = _make(gpu_device)
    lokr = [t for t in L.all_kinds_terms(cfg, w, seed=31) if "attn" in t.name]
    lora = [t for t in _terms(cfg, w, rank=24, seed=32) if "mlp" in t.name]
    dit.set_adapters(lora + lokr)   # (ace355_dit_set_adapters_mixed)
    want = _all_bits(dit, cfg)
    dit.clear_adapters()
    assert _dora_call(dit, lora, lokr) == 0
    assert _same(_all_bits(dit, cfg), want)
    assert _dora_call(dit) == 0
    _, _, fresh = _make(gpu_device)
    assert _same(_all_bits(dit, cfg), _all_bits(fresh, cfg))
    dit.close()
    fresh.close()


def test_graph_replay_after_a_dora_merge(gpu_device):
    from ace355.dit import generate_latents
    cfg, w, dit = _make(gpu_device)
    null, enc, ctx, kw = _sampler_case(cfg)
    kw = dict(kw, infer_steps=8)
    dit.set_graph(True)
    ga = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()   # captured on the base weights
    st = dit.graph_stats()
    dit.set_adapters(_with_dora(L.all_kinds_terms(cfg, w, seed=41, rel_size=1.0), w, seed=42))
    gb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    st2 = dit.graph_stats()
    assert st2["captures"] == st["captures"] and st2["replays"] == st["replays"] + 1, (st, st2)
    tw = _twin(gpu_device, cfg, w, dit)
    tw.set_graph(True)
    ref = generate_latents(tw, null, enc, ctx, **kw)["target_latents"].cpu()
    assert torch.equal(gb, ref) and not torch.equal(ga, gb), "graph replay after the DoRA merge"


def test_stale_slots_and_refusals(gpu_device):
    from ace355 import native
    cfg, w, dit = _make(gpu_device)
    x, ctx, enc, t, tr = _fwd_inputs(cfg)
    for n in range(3):
        dit.set_condition(n, enc[n])
    shapes = cfg.weight_shapes()
    g = torch.Generator().manual_seed(51)
    kname, qname = "layers.0.cross_attn.k_proj.weight", "layers.0.self_attn.q_proj.weight"
    kterm = L.make_term(kname, shapes[kname], (8, 8, 0, 8), g, w0=w[kname])
    kdora = D.make_dora(kname, _w0(w)[kname], [kterm], False, 1.0, D.EPS_BF16, g)
    dit.set_adapters([kterm])
    for n in range(3):
        dit.set_condition(n, enc[n])
    dit.set_adapters([kterm, kdora])   # the DoRA term alone rewrites cross-attention k again: the slots are stale again
    with pytest.raises(RuntimeError, match="slot 0 is stale"):
        dit.forward(x, ctx, t, tr, [0, 1, 2])
    for n in range(3):
        dit.set_condition(n, enc[n])
    assert torch.isfinite(dit.forward(x, ctx, t, tr, [0, 1, 2])).all()
    with pytest.raises(RuntimeError, match="code 3"):
        dit.set_precision("mxfp8")
    with pytest.raises(RuntimeError, match="code 3"):
        dit.set_precision("fp8_weight_only")
    before = _all_bits(dit, cfg)

    # ERR_INVALID, each through the C ABI: one good call with one thing wrong
    qterm = L.make_term(qname, shapes[qname], (16, 16, 0, 0), g, w0=w[qname])
    gq = torch.ones(256, device=gpu_device)
    P = native.ptr

    def row(name=qname, g_=P(gq), per_input=0, eps=2.0 ** -7, m=1.0):
        return native.DoraTermC(name.encode(), g_, per_input, eps, m)
    bad = {
        "two DoRA terms on one target": [row(), row(per_input=1)],
        "no additive term on the target": [row(name="layers.1.self_attn.q_proj.weight")],
        "null g": [row(g_=0)],
        "negative eps": [row(eps=-1.0)],
        "infinite eps": [row(eps=float("inf"))],
        "nan eps": [row(eps=float("nan"))],
        "infinite multiplier": [row(m=float("inf"))],
        "nan multiplier": [row(m=float("nan"))],
        "per_input outside {0, 1}": [row(per_input=2)],
        "unknown target": [row(name="time_embed.linear_2.weight")],
    }
    for what, rows in bad.items():
        assert _dora_call(dit, [], [qterm], rows) == 1, what
        assert _same(_all_bits(dit, cfg), before), f"a refused call changed the weights ({what})"
    with pytest.raises(ValueError, match="does not hold"):   # the Python side checks the shape of g before the call
        dit.set_adapters([qterm, kdora._replace(name=qname)])
    with pytest.raises(RuntimeError, match="code 1"):
        dit.set_adapters([qterm, D.make_dora(kname, _w0(w)[kname], [kterm], False, 1.0, 0.0, g)])
    assert _same(_all_bits(dit, cfg), before)
    # accepted: the good call, and a DoRA term at multiplier 0 on a target without an additive term
    assert _dora_call(dit, [], [qterm], [row(), row(name="layers.1.self_attn.q_proj.weight", m=0.0)]) == 0
    assert not _same(_all_bits(dit, cfg), before)
    dit.clear_adapters()
    dit.set_precision("mxfp8")
    with pytest.raises(RuntimeError, match="quantized"):
        dit.set_adapters([kterm, kdora])
    dit.close()
    _, _, wo = _make(gpu_device)   # (fp8_weight_only needs a handle that was never in mxfp8)
    wo.set_precision("fp8_weight_only")
    with pytest.raises(RuntimeError, match="quantized"):
        wo.set_adapters([kterm, kdora])
    wo.close()


def _handler_case(gpu_device):
    import ace355
    from ace355 import weightgen
    from ace355.backend import NativeHandler
    cfg = ace355.DitConfig(**TINY)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=11, mode="test")
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=11)
    vcfg = ace355.VaeConfig(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    vw = weightgen.make_vae_weights(vcfg.weight_shapes(), seed=1, mode="test")

    def handler(weights):
        h = NativeHandler()
        msg, ok = h.initialize_service(cfg, weights, null, vae_config=vcfg, vae_state_dict=vw, device="cuda")
        assert ok, msg
        return h
    _, enc, ctx, _ = _sampler_case(cfg)

    def run(hh):
        res = hh.generate_music(enc, ctx, seed=[1, 2], inference_steps=27, guidance_scale=7.0)
        assert res["success"], res.get("error")
        return res["extra_outputs"]["pred_latents"].float()

    def twin_of(h):   # a handler that loads the first one's live (merged) weights: loading those bf16 values is exact
        sd = dict(w)
        for n in (f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in KINDS):
            sd[n] = h.native_dit.read_weight(n).cpu()
        return handler(sd)
    return cfg, w, handler, run, twin_of


def test_handler_end_to_end_lokr(gpu_device, tmp_path):
    from safetensors.torch import load_file, save_file
    cfg, w, handler, run, twin_of = _handler_case(gpu_device)
    h = handler(w)
    base = run(h)
    path = str(tmp_path / "style")
    terms = _write_lokr(path, cfg, w)   # (scale 0.5 each, the factors as the merge holds them)
    file = os.path.join(path, "lokr_weights.safetensors")
    sd, g = load_file(file), torch.Generator().manual_seed(71)
    dora = {}
    for i, t in enumerate(terms):
        d = D.make_dora(t.name, _w0(w)[t.name], [t], i % 2 == 1, 1.0, D.EPS_BF16, g)
        dora[t.name] = d
        sd["lycoris_" + t.name[: -len(".weight")].replace(".", "_") + ".dora_scale"] = d.g.reshape((1, -1) if d.per_input else (-1, 1)).contiguous()
    save_file(sd, file, metadata={"lokr_config": json.dumps({"linear_dim": 8, "linear_alpha": 4, "factor": 8, "weight_decompose": True})})
    assert h.add_lora(path).startswith("✅ LoRA 'style' loaded") and h._adapter_type == "lokr"
    full = run(h)
    assert _drift.rel(full, base) > 0.05, "the adapter did not change the latents"
    assert h.set_lora_scale(0.5) == "✅ LoKr scale (style): 0.50"
    half = run(h)
    for t in terms:   # m = 0.5 enters the Kronecker scale and the interpolation
        D.gate(h.native_dit.read_weight(t.name, torch.bfloat16).cpu(), _w0(w)[t.name], [t._replace(scale=0.25)],
               dora[t.name]._replace(scale=0.5), ("handler at 0.5", t.name))
    tw = twin_of(h)
    assert torch.equal(run(tw), half) and not torch.equal(half, full) and not torch.equal(half, base)
    assert h.set_use_lora(False) == "✅ LoKr disabled" and torch.equal(run(h), base)
    assert h.set_use_lora(True) == "✅ LoKr enabled" and torch.equal(run(h), half)
    assert h.unload_lora() == "✅ LoRA unloaded, using base model" and torch.equal(run(h), base) and h._adapter_type is None


def test_handler_end_to_end_peft(gpu_device, tmp_path):
    from safetensors.torch import load_file, save_file
    cfg, w, handler, run, twin_of = _handler_case(gpu_device)
    h = handler(w)
    base = run(h)
    path = str(tmp_path / "style")
    terms = _write_peft(path, cfg, w)   # (name -> LoraTerm at scale 1, bf16-valued B)
    file = os.path.join(path, "adapter_model.safetensors")
    sd, g = load_file(file), torch.Generator().manual_seed(72)
    dora = {}
    for name, t in terms.items():
        a = t._replace(A=t.A.to(torch.bfloat16).float())
        terms[name] = a
        dora[name] = D.make_dora(name, _w0(w)[name], [a._replace(scale=0.5)], False, 1.0, 0.0, g)   # magnitudes around the norms at 0.5
        sd[f"base_model.model.{name[: -len('.weight')]}.lora_magnitude_vector"] = dora[name].g.contiguous()
    save_file(sd, file)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": 8, "lora_alpha": 8, "bias": "none", "use_dora": True}, f)
    assert h.add_lora(path).startswith("✅ LoRA 'style' loaded") and h._adapter_type == "lora"
    full = run(h)
    assert _drift.rel(full, base) > 0.05, "the adapter did not change the latents"
    assert h.set_lora_scale(0.5) == "✅ LoRA scale (style): 0.50"
    half = run(h)
    for name, t in terms.items():   # the user's scale changes s only: m stays 1
        D.gate(h.native_dit.read_weight(name, torch.bfloat16).cpu(), _w0(w)[name], [t._replace(scale=0.5)], dora[name], ("handler at 0.5", name))
    tw = twin_of(h)
    assert torch.equal(run(tw), half) and not torch.equal(half, full) and not torch.equal(half, base)
    assert h.set_use_lora(False) == "✅ LoRA disabled" and torch.equal(run(h), base)
    assert h.set_use_lora(True) == "✅ LoRA enabled" and torch.equal(run(h), half)
    assert h.unload_lora() == "✅ LoRA unloaded, using base model" and torch.equal(run(h), base)
