"""GPU: LoKr adapters merged into the packed DiT weights (ace355_dit_set_adapters_mixed) - merge exactness under the derived gate of
tests/_lokr_cases.py (every element within ulp / 2 + E of the float64 merge and bit-equal to its bf16 rounding away from rounding ties),
parity against the oracle on the merged fp32 weights under the LoRA tests' effect-size rule, bit identity across the adapter lifecycle
(set / clear, LoRA <-> LoKr swaps against fresh twins, the n_kron = 0 call against ace355_dit_set_adapters, graph replay), stale
condition slots, every refusal, and the handler end to end from a lokr_weights.safetensors file."""
import json
import os
import time

import pytest
import torch

import _drift
import _lokr_cases as L
from test_lora_gpu import KINDS, TINY, _bits, _effect_rule, _fwd_inputs, _make, _sampler_case, _terms, _twin

pytestmark = pytest.mark.gpu


def _names(cfg):
    return [f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in KINDS]


def test_merge_exactness_tiny(gpu_device):
    cfg, w, dit = _make(gpu_device)
    base = {n: dit.read_weight(n, torch.bfloat16).cpu() for n in _names(cfg)}
    for label, terms in L.tiny_cases(cfg, w):
        dit.set_adapters(terms)
        mine = L.by_target(terms)
        for n in base:
            got = dit.read_weight(n, torch.bfloat16).cpu()
            if n not in mine:
                assert torch.equal(_bits(got), _bits(base[n])), f"untouched {n} changed ({label})"
                continue
            L.gate(got, base[n], mine[n], (label, n))
    dit.clear_adapters()
    for n, b in base.items():
        assert torch.equal(_bits(dit.read_weight(n, torch.bfloat16).cpu()), _bits(b)), n
    dit.close()


def _default_lokr_terms(cfg, device, kinds, scale=2.0):
    """The reference's default LoKr configuration (LoKRConfig: linear_dim 64, linear_alpha 128, factor -1, W1 full) on ``kinds`` of
    every layer: the near-square split of each dimension, W2 decomposed at rank 64 where 64 < max(out_k, in_n) / 2 and full otherwise
    (the rule of the published LokrModule).  Unit-normal factors on the device, the b factor scaled by r^-1/2."""
    from ace355.lokr import KronTerm

    def near_square(n):
        a = int(n ** 0.5)
        while n % a:
            a -= 1
        return a, n // a   # a <= b
    g = torch.Generator(device=device).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    terms = []
    for name, shape in cfg.weight_shapes().items():
        if not (name.startswith("layers.") and any(name.endswith(k + ".weight") for k in kinds)):
            continue
        o, i = shape
        (out_l, out_k), (in_m, in_n) = near_square(o), near_square(i)
        w1 = rn(out_l, in_m).to(torch.bfloat16)
        if 64 < max(out_k, in_n) / 2:
            terms.append(KronTerm(name, w1, None, None, None, rn(out_k, 64).to(torch.bfloat16), (rn(64, in_n) / 8).to(torch.bfloat16), scale * 1e-3))
        else:
            terms.append(KronTerm(name, w1, None, None, rn(out_k, in_n).to(torch.bfloat16), None, None, scale * 1e-3))
    return terms


def test_merge_full_size_fresh_handle(gpu_device):
    """The real architecture on a FRESH handle: the default LoKr configuration (q / k / v / o of both attentions, 24 layers); the gate
    on the eight kinds of three layers."""
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    cfg = ace355.DitConfig()
    dit = NativeDit(cfg, gpu_device)
    for name, shape in cfg.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
        native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
    native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
    attn = [k for k in KINDS if "attn" in k]
    terms = _default_lokr_terms(cfg, gpu_device, attn)
    assert len(terms) == 8 * cfg.num_hidden_layers
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dit.set_adapters(terms)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    print(f"full size, default LoKr configuration (q/k/v/o of both attentions x 24 layers): set_adapters {ms[0]:.2f} ms (first: + pristine "
          f"copies), then {ms[1]:.2f} / {ms[2]:.2f} ms")
    by = L.by_target(terms)
    for li in (0, 11, 23):
        for k in attn:
            name = f"layers.{li}.{k}.weight"
            w0 = weightgen.make_dit_weights({name: cfg.weight_shapes()[name]}, cfg.hidden_size, seed=4, mode="test")[name]
            L.gate(dit.read_weight(name, torch.bfloat16), w0.to(torch.bfloat16).to(gpu_device), by[name], name, tie_cap=0.05)
    dit.close()


def test_tiny_forward_with_lokr_vs_oracle(gpu_device):
    from oracle import dit as o_dit
    cfg, w, dit = _make(gpu_device)
    terms = L.all_kinds_terms(cfg, w, seed=3, rel_size=1.5)
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
    wm = L.merged(w, terms)
    ref_b, ref_l = o_dit.dit_forward(oc, w, *args), o_dit.dit_forward(oc, wm, *args)
    emu_b, emu_l = _drift.emulated(o_dit.dit_forward, oc, w, *args), _drift.emulated(o_dit.dit_forward, oc, wm, *args)
    _effect_rule("tiny forward, LoKr on ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def test_tiny_sampler_with_lokr_vs_oracle(gpu_device):
    from ace355.dit import generate_latents
    from oracle import dit as o_dit, sampler as o_sampler
    cfg, w, dit = _make(gpu_device)
    terms = L.all_kinds_terms(cfg, w, seed=4, rel_size=1.5)
    null, enc, ctx, kw = _sampler_case(cfg)
    hb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    dit.set_adapters(terms)
    hl = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    oc, wm = o_dit.DitConfig(**TINY), L.merged(w, terms)
    ref_b, ref_l = o_sampler.generate_audio(oc, w, null, enc, ctx, **kw), o_sampler.generate_audio(oc, wm, null, enc, ctx, **kw)
    emu_b = _drift.emulated(o_sampler.generate_audio, oc, w, null, enc, ctx, **kw)
    emu_l = _drift.emulated(o_sampler.generate_audio, oc, wm, null, enc, ctx, **kw)
    _effect_rule("tiny sampler 27 steps CFG 7 + APG, LoKr on ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def _all_bits(dit, cfg):
    return {n: _bits(dit.read_weight(n, torch.bfloat16).cpu()) for n in _names(cfg)}


def _same(a, b):
    return all(torch.equal(a[n], b[n]) for n in a)


def test_lifecycle_bits(gpu_device):
    """set -> clear gives the base bits; a second identical call is bit-identical; LoRA -> LoKr -> LoRA swaps equal fresh twins."""
    cfg, w, dit = _make(gpu_device)
    base = _all_bits(dit, cfg)
    lokr = L.all_kinds_terms(cfg, w, seed=21)
    part = [t for t in L.all_kinds_terms(cfg, w, seed=22, split=(2, 4, 0, 3)) if "q_proj" in t.name or "down_proj" in t.name]
    lora = _terms(cfg, w, rank=8, seed=23)

    def fresh(terms):
        _, _, d = _make(gpu_device)
        d.set_adapters(terms)
        bits = _all_bits(d, cfg)
        d.close()
        return bits
    f_lokr, f_lora, f_part = fresh(lokr), fresh(lora), fresh(part)
    dit.set_adapters(lokr)
    a = _all_bits(dit, cfg)
    dit.set_adapters(lokr)
    assert _same(a, _all_bits(dit, cfg)) and _same(a, f_lokr) and not _same(a, base) and dit.adapters_applied
    dit.clear_adapters()
    assert _same(_all_bits(dit, cfg), base) and not dit.adapters_applied
    dit.set_adapters(lora)
    assert _same(_all_bits(dit, cfg), f_lora)
    dit.set_adapters(part)   # (every other target goes back to its base in the LoKr launch)
    assert _same(_all_bits(dit, cfg), f_part)
    dit.set_adapters(lora)
    assert _same(_all_bits(dit, cfg), f_lora)
    mixed = [t for t in lora if "mlp" in t.name] + [t for t in lokr if "attn" in t.name]   # both families in one call, disjoint targets
    dit.set_adapters(mixed)
    m = _all_bits(dit, cfg)
    assert all(torch.equal(m[n], (f_lora if "mlp" in n else f_lokr)[n]) for n in m)
    dit.set_adapters([t._replace(scale=0.0) for t in lokr])
    assert _same(_all_bits(dit, cfg), base) and not dit.adapters_applied
    dit.close()


def _mixed_call(dit, lora_terms, kron_rows=()):
    """ace355_dit_set_adapters_mixed through ctypes: lora_terms as LoraTerm (moved to the device here), kron_rows as KronTermC rows."""
    from ace355 import native
    keep, rows = [], []
    for t in lora_terms:
        a, b = t.A.to(dit.device, torch.bfloat16).contiguous(), t.B.to(dit.device, torch.bfloat16).contiguous()
        keep += [a, b]
        rows.append(native.LoraTermC(t.name.encode(), native.ptr(a), native.ptr(b), a.shape[0], float(t.scale)))
    arr = (native.LoraTermC * max(len(rows), 1))(*rows)
    karr = (native.KronTermC * max(len(kron_rows), 1))(*kron_rows)
    with torch.cuda.device(dit.device):
        return dit._lib.ace355_dit_set_adapters_mixed(dit._h, arr, len(rows), karr, len(kron_rows), native.current_stream_ptr())


def test_mixed_call_without_kron_terms_is_set_adapters(gpu_device):
    cfg, w, dit = _make(gpu_device)
    lora = _terms(cfg, w, rank=24, seed=31)
    dit.set_adapters(lora)
    want = _all_bits(dit, cfg)
    dit.clear_adapters()
    assert _mixed_call(dit, lora) == 0
    assert _same(_all_bits(dit, cfg), want)
    assert _mixed_call(dit, []) == 0
    _, _, fresh = _make(gpu_device)
    assert _same(_all_bits(dit, cfg), _all_bits(fresh, cfg))
    dit.close()
    fresh.close()


def test_graph_replay_after_a_lokr_merge(gpu_device):
    from ace355.dit import generate_latents
    cfg, w, dit = _make(gpu_device)
    null, enc, ctx, kw = _sampler_case(cfg)
    kw = dict(kw, infer_steps=8)
    dit.set_graph(True)
    ga = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()   # captured on the base weights
    st = dit.graph_stats()
    dit.set_adapters(L.all_kinds_terms(cfg, w, seed=41, rel_size=1.0))
    gb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    st2 = dit.graph_stats()
    assert st2["captures"] == st["captures"] and st2["replays"] == st["replays"] + 1, (st, st2)
    tw = _twin(gpu_device, cfg, w, dit)
    tw.set_graph(True)
    ref = generate_latents(tw, null, enc, ctx, **kw)["target_latents"].cpu()
    assert torch.equal(gb, ref) and not torch.equal(ga, gb), "graph replay after the LoKr merge"


def test_stale_slots_and_refusals(gpu_device):
    from ace355 import native
    cfg, w, dit = _make(gpu_device)
    x, ctx, enc, t, tr = _fwd_inputs(cfg)
    for n in range(3):
        dit.set_condition(n, enc[n])
    shapes = cfg.weight_shapes()
    g = torch.Generator().manual_seed(51)
    kname = "layers.0.cross_attn.k_proj.weight"
    kterm = L.make_term(kname, shapes[kname], (8, 8, 0, 8), g, w0=w[kname])
    dit.set_adapters([kterm])
    with pytest.raises(RuntimeError, match="slot 0 is stale"):
        dit.forward(x, ctx, t, tr, [0, 1, 2])
    for n in range(3):
        dit.set_condition(n, enc[n])
    assert torch.isfinite(dit.forward(x, ctx, t, tr, [0, 1, 2])).all()
    with pytest.raises(RuntimeError, match="code 3"):
        dit.set_precision("mxfp8")
    with pytest.raises(RuntimeError, match="code 3"):
        dit.set_precision("fp8_weight_only")
    with pytest.raises(RuntimeError, match="code 3"):
        dit.load_state_dict(w)
    before = _all_bits(dit, cfg)

    # ERR_INVALID, each through the C ABI: the arguments below are one good term with one thing wrong
    dev = lambda x_: x_.to(gpu_device, torch.bfloat16).contiguous()
    qn = "layers.0.self_attn.q_proj.weight"
    w1, w2, w2a, w2b = dev(torch.randn(16, 16)), dev(torch.randn(16, 16)), dev(torch.randn(16, 4)), dev(torch.randn(4, 16))
    P = native.ptr

    def row(name=qn, w1_=P(w1), w1a=0, w1b=0, w2_=P(w2), w2a_=0, w2b_=0, dims=(16, 16, 16, 16), r1=0, r2=0, scale=0.5):
        return native.KronTermC(name.encode(), w1_, w1a, w1b, w2_, w2a_, w2b_, *dims, r1, r2, scale)
    assert _mixed_call(dit, [], [row(), row(w2_=0, w2a_=P(w2a), w2b_=P(w2b), r2=4)]) == 0   # (the good terms are accepted)
    dit.set_adapters([kterm])
    bad = {
        "out_l x out_k != out": row(dims=(16, 8, 16, 16)),
        "in_m x in_n != in": row(dims=(16, 16, 16, 8)),
        "zero dimension": row(dims=(0, 16, 16, 16)),
        "missing w1": row(w1_=0),
        "missing w2": row(w2_=0),
        "doubled w2": row(w2a_=P(w2a), w2b_=P(w2b), r2=4),
        "half a decomposed factor": row(w2_=0, w2a_=P(w2a), r2=4),
        "decomposed factor of rank 0": row(w2_=0, w2a_=P(w2a), w2b_=P(w2b), r2=0),
        "full factor with a rank": row(r2=4),
        "rank below 0": row(r1=-1),
        "infinite scale": row(scale=float("inf")),
        "nan scale": row(scale=float("nan")),
        "unknown target": row(name="time_embed.linear_2.weight"),
    }
    for what, r in bad.items():
        assert _mixed_call(dit, [], [r]) == 1, what
    lora_q = _terms(cfg, w, rank=4, seed=52, kinds=("self_attn.q_proj",), layers=[0])
    assert _mixed_call(dit, lora_q, [row()]) == 1, "a target named by a LoRA term and a Kronecker term"
    assert "LoRA term and by a Kronecker term" in native.last_error()
    assert _same(_all_bits(dit, cfg), before), "a refused call changed the weights"
    assert _mixed_call(dit, lora_q, [row(name="layers.1.self_attn.q_proj.weight")]) == 0   # disjoint targets: accepted
    dit.clear_adapters()
    dit.set_precision("mxfp8")
    with pytest.raises(RuntimeError, match="quantized"):
        dit.set_adapters([kterm])


def _write_lokr(path, cfg, w, seed=61, rel_size=3.0):
    """lokr_weights.safetensors with lokr_config metadata (linear_dim 8, linear_alpha 4: scale 0.5) on all ten kinds; returns the terms
    as the merge holds them (bf16 factors)."""
    from safetensors.torch import save_file
    terms = L.all_kinds_terms(cfg, w, seed=seed, rel_size=rel_size)
    sd, out = {}, []
    for t in terms:
        m = "lycoris_" + t.name[: -len(".weight")].replace(".", "_")
        k = (t.scale / 0.5) ** 0.5   # the file's scale is alpha / dim = 0.5: the rest of the term's scale lives in the factors
        w1, w2a = (t.w1 * k).to(torch.bfloat16), (t.w2_a * k).to(torch.bfloat16)
        sd[f"{m}.lokr_w1"], sd[f"{m}.lokr_w2_a"], sd[f"{m}.lokr_w2_b"] = w1.contiguous(), w2a.contiguous(), t.w2_b.to(torch.bfloat16).contiguous()
        sd[f"{m}.alpha"] = torch.tensor(4.0)
        out.append(t._replace(w1=w1.float(), w2_a=w2a.float(), scale=0.5))
    os.makedirs(path, exist_ok=True)
    save_file(sd, os.path.join(path, "lokr_weights.safetensors"),
              metadata={"lokr_config": json.dumps({"linear_dim": 8, "linear_alpha": 4, "factor": 8})})
    return out


def test_handler_end_to_end(gpu_device, tmp_path):
    import ace355
    from ace355 import weightgen
    from ace355.backend import NativeHandler
    cfg = ace355.DitConfig(**TINY)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=11, mode="test")
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=11)
    vkw = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    vcfg = ace355.VaeConfig(**vkw)
    vw = weightgen.make_vae_weights(vcfg.weight_shapes(), seed=1, mode="test")

    def handler(weights):
        h = NativeHandler()
        msg, ok = h.initialize_service(cfg, weights, null, vae_config=vcfg, vae_state_dict=vw, device="cuda")
        assert ok, msg
        return h
    h = handler(w)
    _, enc, ctx, _ = _sampler_case(cfg)
    kw = dict(seed=[1, 2], inference_steps=27, guidance_scale=7.0)

    def run(hh):
        res = hh.generate_music(enc, ctx, **kw)
        assert res["success"], res.get("error")
        return res["extra_outputs"]["pred_latents"].float()
    base = run(h)
    terms = _write_lokr(str(tmp_path / "style"), cfg, w)
    assert h.add_lora(str(tmp_path / "style")).startswith("✅ LoRA 'style' loaded")
    assert h._adapter_type == "lokr" and h.get_lora_status()["adapter_type"] == "lokr"
    full = run(h)
    assert _drift.rel(full, base) > 0.05, "the adapter did not change the latents"
    assert h.set_lora_scale(0.5) == "✅ LoKr scale (style): 0.50"
    half = run(h)
    # a twin handle that loads the merged weights directly: the first handle's live weights are bf16_rne(W0 + 0.5 x 0.5 kron) under the
    # gate, and loading those bf16 values is exact
    dit = h.native_dit
    for n in (f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in KINDS):
        t = [x for x in terms if x.name == n]
        L.gate(dit.read_weight(n, torch.bfloat16).cpu(), w[n].to(torch.bfloat16), [x._replace(scale=0.25) for x in t], ("handler at 0.5", n))
    sd = dict(w)
    for li in range(cfg.num_hidden_layers):
        for k in KINDS:
            sd[f"layers.{li}.{k}.weight"] = dit.read_weight(f"layers.{li}.{k}.weight").cpu()
    tw = handler(sd)
    assert torch.equal(run(tw), half) and not torch.equal(half, full) and not torch.equal(half, base)
    assert h.set_use_lora(False) == "✅ LoKr disabled" and torch.equal(run(h), base)
    assert h.set_use_lora(True) == "✅ LoKr enabled" and torch.equal(run(h), half)
    assert h.unload_lora() == "✅ LoRA unloaded, using base model" and torch.equal(run(h), base) and h._adapter_type is None
    assert h.load_lora(str(tmp_path / "style")) == f"✅ LoKr loaded from {tmp_path / 'style' / 'lokr_weights.safetensors'}"
    assert torch.equal(run(h), full)
