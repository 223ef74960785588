"""GPU: cross-attention maps for lyric alignment (ace355_dit_cross_attention_maps, xattn_probs.hip) - the bare kernel against fp64, the
tiny config against the oracle under the 8(d) rule, the full size against the reference fixture G18, the early exit, no state leaking into
later forwards / sampler calls, adapters, refusals, and the handler end to end."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import _drift
from _xattn_capture import capture_cross, checksum, g18_inputs, g18_score_rows, handler_layout

pytestmark = pytest.mark.gpu

TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
TINY_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _make(device, seed=2, cfg_kw=TINY):
    import ace355
    from ace355 import weightgen
    from ace355.dit import NativeDit
    cfg = ace355.DitConfig(**cfg_kw)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=seed, mode="test")
    dit = NativeDit(cfg, device)
    dit.load_state_dict(w)
    return cfg, w, dit


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. bare kernel vs fp64
@pytest.mark.parametrize("Hq,Hkv,heads", [(2, 1, [1]), (2, 1, [0, 1]), (16, 8, [0, 5, 6, 15])])
def test_kernel_vs_fp64(gpu_device, Hq, Hkv, heads):
    from ace355 import native
    lib = native.lib()
    N, scale = 2, 128 ** -0.5
    g = torch.Generator().manual_seed(Hq + len(heads))
    for Sq in (1, 61, 375):
        for Skv in (1, 37, 64, 203, 769, 2304):
            q = (2.0 * torch.randn(N * Sq, Hq * 128, generator=g)).to(torch.bfloat16).to(gpu_device)
            k = (2.0 * torch.randn(N * Skv, Hkv * 128, generator=g)).to(torch.bfloat16).to(gpu_device)
            hs = (C.c_int32 * len(heads))(*heads)
            outs = []
            for _ in range(2):
                out = torch.full((len(heads), N, Skv, Sq), float("nan"), device=gpu_device)
                native.check(lib.ace355_cross_attention_probs(native.ptr(q), native.ptr(k), native.ptr(out), N, Sq, Skv, Hq, Hkv, Hq * 128,
                                                              Hkv * 128, hs, len(heads), scale, native.current_stream_ptr()), "probs")
                outs.append(out)
            torch.cuda.synchronize()
            qd, kd = q.double().view(N, Sq, Hq, 128), k.double().view(N, Skv, Hkv, 128)
            for p, h in enumerate(heads):
                ref = torch.softmax(qd[:, :, h] @ kd[:, :, h // (Hq // Hkv)].transpose(1, 2) * scale, dim=-1).transpose(1, 2)
                err = float((outs[0][p].double() - ref).abs().max())
                assert err <= 1e-5, (Sq, Skv, h, err)
            assert float((outs[0].double().sum(2) - 1).abs().max()) <= 1e-5, (Sq, Skv)
            assert torch.equal(_bits(outs[0]), _bits(outs[1])), (Sq, Skv)


# ------------------------------------------------------------------------------------------------ 2. tiny config vs the oracle
def _oracle_maps(ocfg, w, x, t, enc, ctx, prs, emulate=False):
    from oracle import dit as o_dit
    with capture_cross(o_dit) as cap, torch.no_grad():
        if emulate:
            with o_dit.bf16_storage():
                o_dit.dit_forward(ocfg, o_dit.bf16_weights(w), x, t, t, enc, ctx)
        else:
            o_dit.dit_forward(ocfg, w, x, t, t, enc, ctx)
    return handler_layout(cap, prs)


@pytest.mark.parametrize("kind", ["timestamp", "score"])
def test_tiny_vs_oracle(gpu_device, kind):
    from oracle import dit as o_dit
    cfg, w, dit = _make(gpu_device)
    ocfg = o_dit.DitConfig(**TINY)
    pred, noise, ctx, enc = g18_inputs(41, 19, cfg.hidden_size, 55)
    if kind == "score":
        x, t = g18_score_rows(pred, noise)
        ctx = torch.cat([ctx, ctx])
    else:
        x, t = 0.125 * noise + 0.875 * pred, torch.tensor([0.125])
    N = x.shape[0]
    dit.set_condition(0, enc[0])
    got = dit.cross_attention_maps(x, ctx, t.tolist(), t.tolist(), [0] * N, TINY_PAIRS).cpu()
    ref = _oracle_maps(ocfg, w, x, t, enc.expand(N, -1, -1), ctx, TINY_PAIRS)
    emu = _oracle_maps(ocfg, w, x, t, enc.expand(N, -1, -1), ctx, TINY_PAIRS, emulate=True)
    assert got.shape == (4, N, 19, 21)
    for i, pr in enumerate(TINY_PAIRS):
        _drift.check(f"tiny {kind} map {pr}", _drift.rel(got[i], ref[i]), _drift.rel(emu[i], ref[i]))
    dit.close()


# ------------------------------------------------------------------------------------------------ 3. full size vs G18 (the reference)
def test_full_vs_g18(full_dit_seed4, golden_dir):
    import ace355
    from ace355 import weightgen
    from oracle import dit as o_dit
    dit, cfg, null, wsum = full_dit_seed4
    G = np.load(os.path.join(golden_dir, "g18_alignment.npz"))
    assert wsum == pytest.approx(float(G["full_wsum"]), rel=1e-6)
    T, L = int(G["full_T"]), int(G["full_L"])
    pred, noise, ctx, enc = g18_inputs(T, L, cfg.hidden_size, int(G["full_input_seed"]))
    assert np.allclose(checksum(pred, noise, ctx, enc), G["full_input_sums"], rtol=1e-9)
    x, t = g18_score_rows(pred, noise)
    prs = [tuple(int(v) for v in p) for p in G["full_pairs"]]
    dit.set_condition(0, enc[0])
    got = dit.cross_attention_maps(x, torch.cat([ctx, ctx]), t.tolist(), t.tolist(), [0, 0], prs).cpu()
    want = torch.from_numpy(G["full_maps"])
    # the oracle's bf16-storage drift at the fixture's inputs, measured in this run
    ocfg = o_dit.DitConfig(**{k: getattr(cfg, k) for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                                           "num_key_value_heads", "head_dim")},
                           sliding_window=cfg.sliding_window, layer_types=list(cfg.layer_types))
    w = weightgen.make_dit_weights(o_dit.dit_weight_shapes(ocfg), cfg.hidden_size, seed=4, mode="test")
    args = (x, t, torch.cat([enc, enc]), torch.cat([ctx, ctx]), prs)
    ref = _oracle_maps(ocfg, w, *args)
    emu = _oracle_maps(ocfg, w, *args, emulate=True)
    del w
    for i, pr in enumerate(prs):
        _drift.check(f"full map {pr} vs G18", _drift.rel(got[i], want[i]), _drift.rel(emu[i], ref[i]))


# ------------------------------------------------------------------------------------------------ 4. early exit
def test_early_exit(full_dit_seed4):
    from ace355 import align
    dit, cfg, null, _ = full_dit_seed4
    pred, noise, ctx, enc = g18_inputs(121, 203, cfg.hidden_size, 7)
    x, t = g18_score_rows(pred, noise)
    ctx2 = torch.cat([ctx, ctx])
    dit.set_condition(0, enc[0])
    prs = align.pairs(align.DEFAULT_LAYERS_HEADS, cfg)
    a = dit.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
    b = dit.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs + [(23, 15)])
    assert torch.equal(_bits(a), _bits(b[:len(prs)]))
    # GEMM launches, read from the pass plan (native.dit_pass_plan): patchify + 6 per layer (qkv, o, cross q, cross o, gate|up, down) +
    # proj_out for the full forward; the maps call stops after the cross q of the last requested layer
    from ace355 import native
    max_layer = max(l for l, _ in prs)
    L_enc = enc.shape[1]
    heads = [sum(1 for l, _ in prs if l == li) for li in range(cfg.num_hidden_layers)]
    plan_maps = native.dit_pass_plan(cfg, 121, [(0, L_enc, 0)] * 2, map_last=max_layer, map_heads=heads)["gemm_launches"]
    plan_full = native.dit_pass_plan(cfg, 121, [(0, L_enc, 0)] * 2)["gemm_launches"]
    dit.set_profile(True)
    try:
        dit.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
        n_maps = dit.get_profile()["gemm_launches"]
        dit.set_profile(True)
        dit.forward(x, ctx2, t.tolist(), t.tolist(), [0, 0])
        n_full = dit.get_profile()["gemm_launches"]
    finally:
        dit.set_profile(False)
    assert n_maps == plan_maps == 1 + 6 * max_layer + 3 == 40
    assert n_full == plan_full == 1 + 6 * cfg.num_hidden_layers + 1


# ------------------------------------------------------------------------------------------------ 5. no state leaks into later calls
def test_no_leak_into_forward_and_sampler(gpu_device):
    from ace355 import weightgen
    from ace355.dit import schedule
    cfg, w, a = _make(gpu_device)
    _, _, b = _make(gpu_device)
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=2)
    pred, noise, ctx, enc = g18_inputs(41, 19, cfg.hidden_size, 8)
    ts = schedule(4)

    def run(d):
        out = [d.forward(noise, ctx, [0.5], [0.5], [0])]
        for graph in (True, False):
            d.set_graph(graph)
            out.append(d.sample(noise, ctx, ts, 7.0, cond_slot=0, null_slot=1))
        torch.cuda.synchronize()
        return out
    for d in (a, b):
        d.set_condition(0, enc[0])
        d.set_condition(1, null.reshape(1, -1), L=19)
    before_a, before_b = run(a), run(b)
    x, t = g18_score_rows(pred, noise)
    m = a.cross_attention_maps(x, torch.cat([ctx, ctx]), t.tolist(), t.tolist(), [0, 0], TINY_PAIRS)
    assert torch.isfinite(m).all()
    after_a, after_b = run(a), run(b)
    for i in range(3):
        assert torch.equal(_bits(before_a[i]), _bits(before_b[i])), i
        assert torch.equal(_bits(after_a[i]), _bits(after_b[i])), i
        assert torch.equal(_bits(after_a[i]), _bits(before_a[i])), i
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 6. adapters
def test_adapters_match_merged_twin(gpu_device):
    from ace355.lora import LoraTerm
    kw = dict(TINY, num_hidden_layers=8)
    cfg, w, a = _make(gpu_device, seed=5, cfg_kw=kw)
    pred, noise, ctx, enc = g18_inputs(41, 19, cfg.hidden_size, 9)
    x, t = g18_score_rows(pred, noise)
    ctx2 = torch.cat([ctx, ctx])
    prs = [(2, 0), (3, 1), (6, 0), (6, 1)]
    a.set_condition(0, enc[0])   # built before the adapters: stale afterwards
    g = torch.Generator().manual_seed(1)
    shapes = cfg.weight_shapes()
    terms = []
    for li in range(2, 7):
        for k in ("cross_attn.q_proj", "cross_attn.k_proj"):
            name = f"layers.{li}.{k}.weight"
            o, i = shapes[name]
            A, B = torch.randn(8, i, generator=g), torch.randn(o, 8, generator=g)
            terms.append(LoraTerm(name, A, B, 0.25 * float(w[name].norm()) / float((B @ A).norm())))
    a.set_adapters(terms)
    with pytest.raises(RuntimeError, match="code 3"):
        a.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
    a.set_condition(0, enc[0])
    got = a.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
    merged = dict(w)
    for tm in terms:
        merged[tm.name] = a.read_weight(tm.name).cpu()
    _, _, b = _make(gpu_device, seed=5, cfg_kw=kw)
    b.load_state_dict(merged)
    b.set_condition(0, enc[0])
    want = b.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
    base = _make(gpu_device, seed=5, cfg_kw=kw)[2]
    base.set_condition(0, enc[0])
    plain = base.cross_attention_maps(x, ctx2, t.tolist(), t.tolist(), [0, 0], prs)
    assert torch.equal(_bits(got), _bits(want))
    assert _drift.rel(got, plain) > 1e-2   # the adapters do change the maps
    for d in (a, b, base):
        d.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_output_untouched(gpu_device):
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    cfg, w, dit = _make(gpu_device)
    lib = dit._lib
    pred, noise, ctx, enc = g18_inputs(41, 19, cfg.hidden_size, 10)
    x, cx = noise.to(gpu_device).contiguous(), ctx.to(gpu_device).contiguous()
    dit.set_condition(0, enc[0])
    dit.set_condition(1, weightgen.make_null_condition_emb(cfg.hidden_size, seed=2).reshape(1, -1), L=19)   # broadcast
    dit.set_condition(2, torch.randn(23, cfg.hidden_size))                                                     # another L
    out = torch.full((8, 2, 23, 21), float("nan"), device=gpu_device)
    t = (C.c_float * 2)(0.5, 0.5)

    def call(h=dit._h, slots=(0,), pairs=((0, 0),), n_pairs=None, N=None, xp=None, op=None):
        sl = (C.c_int32 * max(len(slots), 1))(*slots)
        flat = [v for p in (pairs or ()) for v in p]
        pa = (C.c_int32 * max(len(flat), 1))(*flat) if pairs is not None else None
        return lib.ace355_dit_cross_attention_maps(h, native.ptr(x) if xp is None else xp, native.ptr(cx), t, t, sl,
                                                   len(slots) if N is None else N, 41, pa,
                                                   len(flat) // 2 if n_pairs is None else n_pairs,
                                                   native.ptr(out) if op is None else op, native.current_stream_ptr())
    assert call() == 0   # (a valid call, into a scratch buffer below)
    out.fill_(float("nan"))
    cases = {"null x": dict(xp=0), "null out": dict(op=0), "null pairs": dict(pairs=None, n_pairs=1), "no pairs": dict(pairs=()),
             "layer": dict(pairs=((2, 0),)), "neg layer": dict(pairs=((-1, 0),)), "head": dict(pairs=((0, 2),)),
             "unsorted": dict(pairs=((1, 0), (0, 1))), "duplicate": dict(pairs=((0, 1), (0, 1))), "N 0": dict(N=0),
             "N 65": dict(slots=tuple([0] * 65)), "broadcast": dict(slots=(1,)), "mixed L": dict(slots=(0, 2))}
    for what, kw in cases.items():
        assert call(**kw) == 1, what
    fresh = NativeDit(cfg, gpu_device)   # not finalized
    assert call(h=fresh._h) == 3
    from ace355.lora import LoraTerm
    name = "layers.0.cross_attn.k_proj.weight"
    o, i = cfg.weight_shapes()[name]
    dit.set_adapters([LoraTerm(name, torch.randn(4, i), torch.randn(o, 4), 0.01)])
    assert call() == 3, "stale slot"
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    fresh.close(); dit.close()


# ------------------------------------------------------------------------------------------------ 8. handler
def _handler(gpu_device, cfg_kw=TINY, seed=2):
    import ace355
    from ace355 import weightgen
    from ace355.backend import NativeHandler
    cfg = ace355.DitConfig(**cfg_kw)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=seed, mode="test")
    vcfg = ace355.VaeConfig(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    vw = weightgen.make_vae_weights(vcfg.weight_shapes(), seed=1, mode="test")
    h = NativeHandler()
    msg, ok = h.initialize_service(cfg, w, weightgen.make_null_condition_emb(cfg.hidden_size, seed=seed), vae_config=vcfg,
                                   vae_state_dict=vw, device="cuda")
    assert ok, msg
    h.custom_layers_config = {0: [1], 1: [0, 1]}
    return h


@pytest.mark.parametrize("bsz", [1, 2])
def test_handler_lyric_attention_composes(gpu_device, bsz):
    from ace355 import align
    h = _handler(gpu_device)
    g = torch.Generator().manual_seed(bsz)
    enc = torch.randn(bsz, 19, 256, generator=g)
    ctx = torch.cat([0.5 * torch.randn(bsz, 41, 64, generator=g), torch.ones(bsz, 41, 64)], -1)
    res = h.generate_music(enc, ctx, seed=[3 + i for i in range(bsz)], inference_steps=4)
    assert res["success"], res.get("error")
    ex = res["extra_outputs"]
    pred, e, c = ex["pred_latents"], ex["encoder_hidden_states"], ex["context_latents"]
    assert not pred.is_cuda
    prs = align.pairs(h.custom_layers_config, h.native_dit.cfg)
    for kind in ("timestamp", "score"):
        got = h.lyric_attention(pred, e, c, inference_steps=8, seed=42, kind=kind)
        p = pred.to(gpu_device, torch.bfloat16)
        x, t = align.alignment_rows(p, align.noise_like(p, 42), 8, kind)
        for b in range(bsz):
            h.native_dit.set_condition(b, e[b].to(gpu_device, torch.bfloat16))
        cc = c.to(gpu_device, torch.bfloat16)
        slots = list(range(bsz)) * (2 if kind == "score" else 1)
        cc = torch.cat([cc, cc]) if kind == "score" else cc
        maps = h.native_dit.cross_attention_maps(x.float(), cc.float(), t.float().tolist(), t.float().tolist(), slots, prs)
        want = align.stack(maps, prs, bsz, 2, torch.bfloat16)
        for gg, ww in zip(got if kind == "score" else [got], want if kind == "score" else [want]):
            assert gg.dtype == torch.bfloat16 and torch.equal(gg.view(torch.int16), ww.view(torch.int16)), kind
    h.native_dit.close()


def test_handler_get_lyric_timestamp(gpu_device, monkeypatch):
    h = _handler(gpu_device)
    seen = {}

    class MusicStampsAligner:
        def __init__(self, tok):
            pass

        def stamps_align_info(self, attention_matrix, **kw):
            seen["m"] = attention_matrix
            return {"calc_matrix": 1}

        def get_timestamps_and_lrc(self, calc_matrix, lyrics_tokens, total_duration_seconds):
            return {"lrc_text": "[00:00.00]x", "sentence_timestamps": [], "token_timestamps": []}
    mod = types.ModuleType("acestep.core.scoring.dit_alignment")
    mod.MusicStampsAligner = MusicStampsAligner
    for name in ("acestep", "acestep.core", "acestep.core.scoring"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.setitem(sys.modules, "acestep.core.scoring.dit_alignment", mod)

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return [0, 0, 0]
    h.text_tokenizer = Tok()
    g = torch.Generator().manual_seed(0)
    r = h.get_lyric_timestamp(torch.randn(1, 41, 64, generator=g), torch.randn(1, 19, 256, generator=g), torch.ones(1, 19),
                              torch.randn(1, 41, 128, generator=g), torch.tensor([[0, 0, 0, 5, 6, 151643]]), 10.0)
    assert r["success"] is True and r["lrc_text"] == "[00:00.00]x" and r["error"] is None
    m = seen["m"]
    assert m.dtype == torch.bfloat16 and m.is_cuda and m.shape == (2, 2, 2, 21)   # [layers, H, lyric rows 3:5 (up to <|endoftext|>), S]
    h.native_dit.close()


@pytest.mark.parametrize("precision", ["fp8_weight_only", "mxfp8"])
def test_quantised_handles_give_probabilities(gpu_device, precision):
    from ace355 import align
    cfg, w, dit = _make(gpu_device)
    dit.set_precision(precision)
    pred, noise, ctx, enc = g18_inputs(41, 19, cfg.hidden_size, 11)
    out = align.lyric_attention(dit, pred, enc, ctx, 8, 42, {0: [0, 1], 1: [1]}, "timestamp", torch.float32)
    assert torch.isfinite(out).all()
    assert float((out[[0, 0, 1], [0, 1, 1]].sum(1) - 1).abs().max()) < 1e-5
    dit.close()
