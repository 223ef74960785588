"""GPU: LoRA adapters merged into the packed DiT weights (ace355_dit_set_adapters) - merge exactness, parity against the oracle on the
merged fp32 weights under the effect-size rule, bit identity across the adapter lifecycle and on every launch path (against a twin
handle loaded with the merged weights), stale condition slots, refusals, and the handler end to end.

Effect-size rule: a LoRA delta can be smaller than the bf16 drift, and a parity test would then pass with the adapter ignored.  Every
parity test therefore asserts that the oracle's own distance between the adapted and the base result is >= 10 x the gate it applies,
and that the adapter's CONTRIBUTION (HIP adapted - HIP base against oracle adapted - oracle base) passes the 8(d) rule applied to the
emulated contribution."""
import json
import os
import time

import pytest
import torch

import _drift

pytestmark = pytest.mark.gpu

TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "cross_attn.q_proj", "cross_attn.k_proj",
         "cross_attn.v_proj", "cross_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _make(device, seed=11, cfg_kw=TINY):
    import ace355
    from ace355 import weightgen
    from ace355.dit import NativeDit
    cfg = ace355.DitConfig(**cfg_kw)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=seed, mode="test")
    dit = NativeDit(cfg, device)
    dit.load_state_dict(w)
    return cfg, w, dit


def _terms(cfg, w, rank=8, seed=0, rel_size=0.25, kinds=KINDS, layers=None):
    """One seeded term per target; the scale makes ||s B A|| = rel_size x ||W0|| (a delta well above the bf16 drift)."""
    from ace355.lora import LoraTerm
    g = torch.Generator().manual_seed(seed)
    shapes = cfg.weight_shapes()
    out = []
    for li in (range(cfg.num_hidden_layers) if layers is None else layers):
        for k in kinds:
            name = f"layers.{li}.{k}.weight"
            o, i = shapes[name]
            A = torch.randn(rank, i, generator=g).to(torch.bfloat16).float()
            B = torch.randn(o, rank, generator=g).to(torch.bfloat16).float()
            s = rel_size * float(w[name].norm()) / float((B @ A).norm())
            out.append(LoraTerm(name, A, B, s))
    return out


def _merged(w, terms):
    """The fp32 dict w0 + sum s B @ A (the oracle's expectation)."""
    m = dict(w)
    for t in terms:
        m[t.name] = (m[t.name].double() + t.scale * (t.B.double() @ t.A.double())).float()
    return m


def _bits(x):
    return x.contiguous().view(torch.int16)


def _check_merge(got, w0, terms, what):
    """got (bf16) against bf16(float64(W0) + sum s B @ A): >= 99.9 % bit-identical, and every element within 1 bf16 ulp of the float64
    value - except where the sum cancels far below its parts: there within the fp32 accumulation's error bound,
    (rank + 2) 2^-24 (|W0| + sum |s| |B| @ |A|)."""
    w0 = w0.double()
    dev = w0.device
    exact, mag = w0.clone(), w0.abs()
    for t in terms:
        B, A = t.B.double().to(dev), t.A.double().to(dev)
        exact += t.scale * (B @ A)
        mag += (A.shape[0] + 2) * abs(t.scale) * (B.abs() @ A.abs())
    exp = exact.to(torch.bfloat16)
    g = got.to(dev)
    same = float((_bits(g) == _bits(exp)).float().mean())
    err = (g.double() - exact).abs()
    ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(1e-38))) - 7)
    allowed = torch.maximum(ulp, 2.0 ** -24 * mag)
    worst = float((err / allowed).max())
    assert worst <= 1.0 and same >= 0.999, (what, worst, same)
    return same


def test_merge_exactness_tiny(gpu_device):
    cfg, w, dit = _make(gpu_device)
    base = {f"layers.{li}.{k}.weight": dit.read_weight(f"layers.{li}.{k}.weight", torch.bfloat16).cpu()
            for li in range(cfg.num_hidden_layers) for k in KINDS}
    for name, b in base.items():   # read_weight is the inverse of the pack row map
        assert torch.equal(b, w[name].to(torch.bfloat16)), name
    for rank in (1, 8, 48, 256):
        terms = _terms(cfg, w, rank=rank, seed=rank, layers=[0])
        extra = _terms(cfg, w, rank=max(1, rank // 2 + 3), seed=100 + rank, kinds=("cross_attn.k_proj",), layers=[0])   # two terms, one target
        dit.set_adapters(terms + extra)
        for name in base:
            got = dit.read_weight(name, torch.bfloat16).cpu()
            mine = [t for t in terms + extra if t.name == name]
            if not mine:
                assert torch.equal(_bits(got), _bits(base[name])), f"untouched {name} changed (rank {rank})"
                continue
            _check_merge(got, w[name].to(torch.bfloat16), mine, (name, rank))
        print(f"rank {rank}: all ten kinds within 1 bf16 ulp of the float64 merge, untouched weights bit-identical")
    dit.clear_adapters()
    for name, b in base.items():
        assert torch.equal(_bits(dit.read_weight(name, torch.bfloat16).cpu()), _bits(b)), name
    dit.close()


def test_merge_full_size_fresh_handle(gpu_device):
    """The real architecture on a FRESH handle: all ten kinds of all 24 layers at rank 64; exactness checked on three layers."""
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    from ace355.lora import LoraTerm
    cfg = ace355.DitConfig()
    dit = NativeDit(cfg, gpu_device)
    for name, shape in cfg.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
        native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
    native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
    g = torch.Generator(device=gpu_device).manual_seed(1)
    terms = []
    for name, shape in cfg.weight_shapes().items():
        if any(name.endswith(k + ".weight") for k in KINDS) and name.startswith("layers."):
            o, i = shape
            A = torch.randn(64, i, device=gpu_device, generator=g).to(torch.bfloat16)
            B = torch.randn(o, 64, device=gpu_device, generator=g).to(torch.bfloat16)
            terms.append(LoraTerm(name, A, B, 1e-3))
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dit.set_adapters(terms)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    print(f"full size, ten kinds x 24 layers, rank 64: set_adapters {ms[0]:.2f} ms (first: + pristine copies), then {ms[1]:.2f} / {ms[2]:.2f} ms")
    for li in (0, 11, 23):
        for k in KINDS:
            name = f"layers.{li}.{k}.weight"
            t = [x for x in terms if x.name == name][0]
            w0 = weightgen.make_dit_weights({name: cfg.weight_shapes()[name]}, cfg.hidden_size, seed=4, mode="test")[name]
            _check_merge(dit.read_weight(name, torch.bfloat16), w0.to(torch.bfloat16).to(gpu_device),
                         [t], name)
    dit.close()


def _fwd_inputs(cfg):
    g = torch.Generator().manual_seed(5)
    N, T, L = 3, 85, 40   # odd T, t_r != t on one row
    x = torch.randn(N, T, 64, generator=g)
    ctx = torch.cat([0.5 * torch.randn(N, T, 64, generator=g), torch.ones(N, T, 64)], -1)
    enc = torch.randn(N, L, cfg.hidden_size, generator=g)
    return x, ctx, enc, [0.9, 0.5, 0.1], [0.9, 0.4, 0.1]


def _effect_rule(what, hip_l, hip_b, ref_l, ref_b, emu_l, emu_b):
    drift = _drift.rel(emu_l, ref_l)
    effect = _drift.rel(ref_l, ref_b)
    gate = _drift.FACTOR * drift
    print(f"    {what}: effect size rel(oracle lora, oracle base) {effect:.3e} = {effect / gate:.1f} x the gate {gate:.3e}")
    assert effect >= 10 * gate, (what, effect, gate)
    _drift.check(f"{what}, adapted result", _drift.rel(hip_l, ref_l), drift)
    _drift.check(f"{what}, adapter contribution", _drift.rel(hip_l - hip_b, ref_l - ref_b), _drift.rel(emu_l - emu_b, ref_l - ref_b))


def test_tiny_forward_with_adapters_vs_oracle(gpu_device):
    from oracle import dit as o_dit
    cfg, w, dit = _make(gpu_device)
    terms = _terms(cfg, w, rank=16, seed=3, rel_size=1.5)
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
    wm = _merged(w, terms)
    ref_b, ref_l = o_dit.dit_forward(oc, w, *args), o_dit.dit_forward(oc, wm, *args)
    emu_b, emu_l = _drift.emulated(o_dit.dit_forward, oc, w, *args), _drift.emulated(o_dit.dit_forward, oc, wm, *args)
    _effect_rule("tiny forward, ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def _sampler_case(cfg):
    from ace355 import weightgen
    g = torch.Generator().manual_seed(7)
    B, T, L = 2, 40, 17
    enc = torch.randn(1, L, cfg.hidden_size, generator=g).expand(B, -1, -1).contiguous()
    ctx = torch.cat([0.5 * torch.randn(B, T, 64, generator=g), torch.ones(B, T, 64)], -1)
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=11)
    return null, enc, ctx, dict(seed=[1, 2], infer_steps=27, diffusion_guidance_sale=7.0)


def test_tiny_sampler_with_adapters_vs_oracle(gpu_device):
    from ace355.dit import generate_latents
    from oracle import dit as o_dit, sampler as o_sampler
    cfg, w, dit = _make(gpu_device)
    terms = _terms(cfg, w, rank=8, seed=4, rel_size=1.5)
    null, enc, ctx, kw = _sampler_case(cfg)
    hb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    dit.set_adapters(terms)
    hl = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    oc, wm = o_dit.DitConfig(**TINY), _merged(w, terms)
    ref_b, ref_l = o_sampler.generate_audio(oc, w, null, enc, ctx, **kw), o_sampler.generate_audio(oc, wm, null, enc, ctx, **kw)
    emu_b = _drift.emulated(o_sampler.generate_audio, oc, w, null, enc, ctx, **kw)
    emu_l = _drift.emulated(o_sampler.generate_audio, oc, wm, null, enc, ctx, **kw)
    _effect_rule("tiny sampler 27 steps CFG 7 + APG, ten kinds", hl, hb, ref_l, ref_b, emu_l, emu_b)


def test_bit_identity_across_the_lifecycle(gpu_device):
    cfg, w, dit = _make(gpu_device)
    a = _terms(cfg, w, rank=8, seed=21)
    b = _terms(cfg, w, rank=24, seed=22, kinds=("self_attn.q_proj", "mlp.down_proj", "cross_attn.v_proj"))
    x, ctx, enc, t, tr = _fwd_inputs(cfg)

    def fwd():
        for n in range(3):
            dit.set_condition(n, enc[n])
        return dit.forward(x, ctx, t, tr, [0, 1, 2]).cpu()
    base = fwd()
    dit.set_adapters(a)
    fa = fwd()
    dit.set_adapters(a + b)
    fab = fwd()
    dit.set_adapters(a)
    fa2 = fwd()
    dit.set_adapters(a)
    fa3 = fwd()
    assert torch.equal(fa, fa2) and torch.equal(fa, fa3) and not torch.equal(fa, fab) and not torch.equal(fa, base)
    assert dit.adapters_applied
    dit.clear_adapters()
    assert torch.equal(fwd(), base) and not dit.adapters_applied
    dit.set_adapters([tt._replace(scale=0.0) for tt in a])
    assert torch.equal(fwd(), base)


def _twin(device, cfg, w, dit):
    """A fresh handle whose weights are the first handle's live (merged) ones."""
    from ace355.dit import NativeDit
    sd = dict(w)
    for li in range(cfg.num_hidden_layers):
        for k in KINDS:
            name = f"layers.{li}.{k}.weight"
            sd[name] = dit.read_weight(name).cpu()
    tw = NativeDit(cfg, device)
    tw.load_state_dict(sd)
    return tw


def test_interactions_against_a_twin(gpu_device):
    from ace355.dit import generate_latents
    cfg, w, dit = _make(gpu_device)
    a = _terms(cfg, w, rank=8, seed=31)
    b = _terms(cfg, w, rank=16, seed=32)
    null, enc, ctx, kw = _sampler_case(cfg)
    kw = dict(kw, infer_steps=8)
    dit.set_adapters(a)
    tw = _twin(gpu_device, cfg, w, dit)

    def both(fn):
        return fn(dit), fn(tw)
    # plain sampler call (one chain)
    for h in (dit, tw):
        h.set_dual(0)
    x, y = both(lambda h: generate_latents(h, null, enc, ctx, **kw)["target_latents"].cpu())
    assert torch.equal(x, y), "plain sampler call"
    # dual-chain 2-song request
    for h in (dit, tw):
        h.set_dual(2)
    n0 = dit.dual_count()
    x, y = both(lambda h: generate_latents(h, null, enc, ctx, **kw)["target_latents"].cpu())
    assert dit.dual_count() == n0 + 1, "the 2-song request did not run as two chains"
    assert torch.equal(x, y), "dual-chain request"
    # layer-0 de-duplication and the weight prefetch of a one-song request (CFG: both on by default, one chain)
    d0 = dit.dedup_count()
    x, y = both(lambda h: generate_latents(h, null, enc[:1], ctx[:1], **dict(kw, seed=[3]))["target_latents"].cpu())
    assert dit.dedup_count() > d0 and torch.equal(x, y), "one-song request (layer-0 dedup, weight prefetch)"
    for h in (dit, tw):
        h.set_dual(1)
    # captured sampler graph: capture with a, switch to b, replay (the merge rewrites the weights in place: no new capture)
    dit.set_graph(True)
    ga = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    st = dit.graph_stats()
    dit.set_adapters(b)
    gb = generate_latents(dit, null, enc, ctx, **kw)["target_latents"].cpu()
    st2 = dit.graph_stats()
    assert st2["captures"] == st["captures"] and st2["replays"] == st["replays"] + 1, (st, st2)
    tw_b = _twin(gpu_device, cfg, w, dit)
    tw_b.set_graph(True)
    ref_b = generate_latents(tw_b, null, enc, ctx, **kw)["target_latents"].cpu()
    assert torch.equal(gb, ref_b) and not torch.equal(ga, gb), "graph replay after the switch to b"


def test_stale_slots_and_refusals(gpu_device):
    cfg, w, dit = _make(gpu_device)
    x, ctx, enc, t, tr = _fwd_inputs(cfg)
    for n in range(3):
        dit.set_condition(n, enc[n])
    dit.set_adapters(_terms(cfg, w, rank=4, seed=41, kinds=("cross_attn.k_proj",)))
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
    with pytest.raises(RuntimeError, match="code 1"):
        dit.set_adapters([_terms(cfg, w, rank=4, seed=42, kinds=("self_attn.q_proj",))[0]._replace(name="time_embed.linear_2.weight")])
    dit.clear_adapters()
    dit.set_precision("mxfp8")
    with pytest.raises(RuntimeError, match="quantized"):
        dit.set_adapters(_terms(cfg, w, rank=4, seed=43, kinds=("self_attn.q_proj",)))


def _write_peft(path, cfg, w, rank=8, seed=51, rel_size=3.0):
    from safetensors.torch import save_file
    terms = _terms(cfg, w, rank=rank, seed=seed, rel_size=rel_size)
    sd = {}
    for t in terms:
        m = t.name[: -len(".weight")]
        sd[f"base_model.model.{m}.lora_A.weight"] = t.A.contiguous()
        sd[f"base_model.model.{m}.lora_B.weight"] = (t.B * t.scale).contiguous()   # alpha / r = 1: the scale lives in B
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": rank, "lora_alpha": rank, "bias": "none"}, f)
    save_file(sd, os.path.join(path, "adapter_model.safetensors"))
    return {t.name: t._replace(B=(t.B * t.scale).to(torch.bfloat16).float(), A=t.A, scale=1.0) for t in terms}


def test_handler_end_to_end(gpu_device, tmp_path):
    import ace355
    from ace355 import weightgen
    from ace355.backend import NativeHandler
    from oracle import dit as o_dit, sampler as o_sampler
    cfg = ace355.DitConfig(**TINY)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=11, mode="test")
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=11)
    vkw = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    vcfg = ace355.VaeConfig(**vkw)
    vw = weightgen.make_vae_weights(vcfg.weight_shapes(), seed=1, mode="test")
    h = NativeHandler()
    msg, ok = h.initialize_service(cfg, w, null, vae_config=vcfg, vae_state_dict=vw, device="cuda")
    assert ok, msg
    _, enc, ctx, _ = _sampler_case(cfg)
    kw = dict(seed=[1, 2], inference_steps=27, guidance_scale=7.0)

    def run():
        res = h.generate_music(enc, ctx, **kw)
        assert res["success"], res.get("error")
        return res["extra_outputs"]["pred_latents"].float()
    base = run()
    terms = _write_peft(str(tmp_path / "style"), cfg, w)
    assert h.add_lora(str(tmp_path / "style")).startswith("✅ LoRA 'style' loaded")
    lo = run()
    assert _drift.rel(lo, base) > 0.05, "the adapter did not change the latents"
    assert h.set_lora_scale(0.0).startswith("✅") and torch.equal(run(), base)
    assert h.set_lora_scale(0.5).startswith("✅")
    half = run()
    oc = o_dit.DitConfig(**TINY)
    wm = _merged(w, [t._replace(scale=0.5) for t in terms.values()])
    okw = dict(seed=[1, 2], infer_steps=27, diffusion_guidance_sale=7.0)
    ref_b, ref_l = o_sampler.generate_audio(oc, w, null, enc, ctx, **okw), o_sampler.generate_audio(oc, wm, null, enc, ctx, **okw)
    # the handler returns its latents in the host dtype (bf16 on the GPU, as the reference does): the emulated side is stored the same way
    emu_b = _drift.emulated(o_sampler.generate_audio, oc, w, null, enc, ctx, **okw).to(torch.bfloat16).float()
    emu_l = _drift.emulated(o_sampler.generate_audio, oc, wm, null, enc, ctx, **okw).to(torch.bfloat16).float()
    _effect_rule("handler generate_music at scale 0.5", half, base, ref_l, ref_b, emu_l, emu_b)
    assert h.set_use_lora(False) == "✅ LoRA disabled" and torch.equal(run(), base)
    assert h.set_use_lora(True) == "✅ LoRA enabled" and torch.equal(run(), half)
    assert h.remove_lora("style") == "✅ LoRA unloaded, using base model" and torch.equal(run(), base)
