"""GPU parity of the native Oobleck decoder (through the C ABI) against the oracle restatement.

The oracle for this part is parity-UNPINNED (third-party diffusers arithmetic, see oracle/oobleck.py); what is
asserted is agreement of the HIP path with that restatement: bf16 activations through ~36 conv layers.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _snr_db(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float(10 * torch.log10(b.pow(2).sum() / ((a - b).pow(2).sum() + 1e-30)))


def _build(cfg_kw, device, seed=1):
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    cfg = ace355.VaeConfig(**cfg_kw)
    w = weightgen.make_vae_weights(cfg.weight_shapes(), seed=seed, mode="test")
    vae = NativeVae(cfg, device)
    vae.load_state_dict(w)
    return cfg, w, vae


@pytest.mark.parametrize("cfg_kw,B,T", [
    (dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6)), 2, 37),
    (dict(), 1, 24),
    (dict(), 2, 9),
])
def test_decode_vs_oracle(gpu_device, cfg_kw, B, T):
    cfg, w, vae = _build(cfg_kw, gpu_device)
    _check_decode_vs_oracle(cfg_kw, cfg, w, vae, B, T)


def test_decode_of_prefused_weights_vs_oracle(gpu_device):
    """The small case of test_decode_vs_oracle on a handle that was given every conv as its pre-fused ``<conv>.weight`` (g v / (||v|| + 1e-9)
    in fp32 on the CPU, the formula of tests/_vae_layers.py) in place of the weight_g / weight_v pair; the oracle keeps the pair."""
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    cfg_kw = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    cfg = ace355.VaeConfig(**cfg_kw)
    w = weightgen.make_vae_weights(cfg.weight_shapes(), seed=1, mode="test")
    fused = {k: t for k, t in w.items() if not k.endswith((".weight_g", ".weight_v"))}
    for k in w:
        if k.endswith(".weight_v"):
            v, g = w[k].float(), w[k[:-1] + "g"].float().reshape(-1, 1, 1)
            nrm = v.double().reshape(v.shape[0], -1).pow(2).sum(1).sqrt().float().reshape(-1, 1, 1)
            fused[k[:-2]] = (g * v) / (nrm + torch.tensor(1e-9, dtype=torch.float32))
    assert len(fused) < len(w) and not any(k.endswith(("_g", "_v")) for k in fused)
    vae = NativeVae(cfg, gpu_device)
    vae.load_state_dict(fused)
    _check_decode_vs_oracle(cfg_kw, cfg, w, vae, 2, 37)


def _check_decode_vs_oracle(cfg_kw, cfg, w, vae, B, T):
    from oracle import oobleck as o_vae
    assert vae.hop == cfg.hop
    g = torch.Generator().manual_seed(T)
    z = torch.randn(B, 64, T, generator=g)
    wav = vae.decode(z)
    assert wav.shape == (B, cfg.audio_channels, cfg.hop * T) and wav.dtype == torch.float32
    o_cfg = o_vae.VaeConfig(**cfg_kw)
    ref = o_vae.decode(o_cfg, w, z)                       # fp32 restatement
    emu = o_vae.decode(o_cfg, w, z, emulate_bf16=True)    # same restatement, bf16 storage between layers, every Snake input rounded
    nat = o_vae.decode(o_cfg, w, z, emulate_bf16="native")  # bf16 storage with the HIP path's rounding points (producer-side Snakes)
    snr_fp32, snr_emu, snr_nat, drift = _snr_db(wav, ref), _snr_db(wav, emu), _snr_db(wav, nat), _snr_db(emu, ref)
    print(f"vae decode {cfg_kw or 'full'} B={B} T={T}: SNR vs fp32 oracle {snr_fp32:.1f} dB, vs bf16-storage oracle "
          f"{snr_emu:.1f} dB, vs the oracle with the native rounding points {snr_nat:.1f} dB (bf16-storage drift of the oracle itself: "
          f"{drift:.1f} dB); wav rms {float(ref.pow(2).mean().sqrt()):.3f}")
    # stated tolerance (SURVEY 8d parity gate): the HIP waveform may differ from the fp32 restatement by at most 2x
    # (6 dB) the drift the restatement shows against itself when it stores activations in bf16 ...
    assert snr_fp32 > drift - 6.0, (snr_fp32, drift)
    # ... and must agree with both bf16-storage restatements (layer-by-layer rounding; the native rounding points) to >= 30 dB.
    assert snr_emu > 30.0 and snr_nat > 30.0, (snr_emu, snr_nat)


def test_decode_at_the_metric_length_vs_oracle(gpu_device):
    """The decode AT THE METRIC LENGTH against the oracle itself (call site generate_music_decode.py:165-177):
    full configuration, T = 750 latent frames (30 s, 1 440 000 samples per channel), B = 1, the whole waveform against
    oracle/oobleck.py in fp32 and with bf16 storage between layers - the gates of test_decode_vs_oracle.  Until round 3 every decode
    longer than 48 frames was only checked against shorter NATIVE decodes: a defect common to all native decodes of a certain size
    (a grid-dimension wrap, a 32-bit offset) would have passed.  ~25 s of oracle time on the GPU box's 16 host threads."""
    from oracle import oobleck as o_vae
    cfg, w, vae = _build(dict(), gpu_device)
    T = 750
    z = torch.randn(1, 64, T, generator=torch.Generator().manual_seed(750))
    wav = vae.decode(z)
    assert wav.shape == (1, cfg.audio_channels, cfg.hop * T) and torch.isfinite(wav).all()
    assert torch.equal(wav, vae.decode(z)), "the same latents twice: not bit-identical"
    # ... and inside the batch the bench decodes (B = 8, this item in slot 5): the same waveform bit for bit
    z8 = torch.randn(8, 64, T, generator=torch.Generator().manual_seed(751))
    z8[5] = z[0]
    assert torch.equal(vae.decode(z8)[5], wav[0]), "an item's waveform depends on the batch it is decoded in"
    o_cfg = o_vae.VaeConfig()
    ref = o_vae.decode(o_cfg, w, z)
    emu = o_vae.decode(o_cfg, w, z, emulate_bf16=True)
    snr_fp32, snr_emu, drift = _snr_db(wav, ref), _snr_db(wav, emu), _snr_db(emu, ref)
    # the worst 1 s stretch as well: a localised defect would hide in a whole-signal SNR
    sec = 48000
    per_sec = [_snr_db(wav[..., i:i + sec], emu[..., i:i + sec]) for i in range(0, wav.shape[-1], sec)]
    print(f"vae decode full config T=750 B=1: SNR vs fp32 oracle {snr_fp32:.1f} dB, vs bf16-storage oracle {snr_emu:.1f} dB (oracle's own "
          f"bf16 drift {drift:.1f} dB); worst second vs bf16-storage oracle {min(per_sec):.1f} dB")
    assert snr_fp32 > drift - 6.0, (snr_fp32, drift)
    assert snr_emu > 30.0 and min(per_sec) > 27.0, (snr_emu, min(per_sec))


def test_long_decode_deep_window_vs_oracle(gpu_device):
    """configs[2]'s length (T = 3000 latent frames, 120 s): the LAST 200 frames of the native whole-sequence decode against the ORACLE
    run on a window deep inside the sequence (frames 2784..3000: 16 halo frames on the left - the decoder's receptive field is 8.9
    latent frames, DESIGN.md section 4 - the true sequence end on the right).  The reference side is the oracle, not a native decode."""
    from oracle import oobleck as o_vae
    cfg, w, vae = _build(dict(), gpu_device)
    T, win, halo = 3000, 200, 16
    z = torch.randn(1, 64, T, generator=torch.Generator().manual_seed(3000))
    wav = vae.decode(z)
    assert wav.shape == (1, cfg.audio_channels, cfg.hop * T) and torch.isfinite(wav).all()
    zc = z[:, :, T - win - halo:].contiguous()
    o_cfg = o_vae.VaeConfig()
    ref = o_vae.decode(o_cfg, w, zc)[..., cfg.hop * halo:]
    emu = o_vae.decode(o_cfg, w, zc, emulate_bf16=True)[..., cfg.hop * halo:]
    got = wav[..., cfg.hop * (T - win):]
    assert got.shape == ref.shape
    snr_fp32, snr_emu, drift = _snr_db(got, ref), _snr_db(got, emu), _snr_db(emu, ref)
    print(f"vae decode full config T=3000, frames 2800-3000 vs the oracle on that window: SNR vs fp32 {snr_fp32:.1f} dB, vs bf16-storage "
          f"{snr_emu:.1f} dB (oracle's own bf16 drift {drift:.1f} dB)")
    assert snr_fp32 > drift - 6.0, (snr_fp32, drift)
    assert snr_emu > 30.0, snr_emu


def test_whole_sequence_equals_tiled(gpu_device):
    """the reference's overlap-discard tiling equals the un-tiled decode away from fp order."""
    from oracle import tiling as o_tiling
    cfg_kw = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    cfg, w, vae = _build(cfg_kw, gpu_device)
    z = torch.randn(1, 64, 200, generator=torch.Generator().manual_seed(3))
    whole = vae.decode(z)
    tiled = o_tiling.tiled_decode(lambda c: vae.decode(c).cpu(), z, chunk_size=96, overlap=24)
    assert tiled.shape == whole.shape
    assert _snr_db(tiled, whole) > 35.0


def test_peak_normalize_and_latent_check(gpu_device):
    from ace355.vae import latent_check, peak_normalize
    from oracle import tiling as o_tiling
    wav = torch.randn(3, 2, 5000, generator=torch.Generator().manual_seed(0))
    wav[1] *= 0.1
    ref = o_tiling.peak_normalize(wav.clone())
    got = peak_normalize(wav.clone().to(gpu_device))
    assert float((got.cpu() - ref).abs().max()) < 1e-6
    quiet = torch.rand(2, 2, 100) * 0.5
    assert torch.equal(peak_normalize(quiet.clone().to(gpu_device)).cpu(), quiet)
    assert latent_check(torch.zeros(4, 5, device=gpu_device)) == (False, True)
    assert latent_check(torch.ones(4, 5, device=gpu_device)) == (False, False)
    bad = torch.ones(4, 5, device=gpu_device)
    bad[1, 2] = float("nan")
    assert latent_check(bad)[0] is True


def test_full_length_decode_properties(gpu_device):
    """Size-independent properties at the metric length (30 s = 750 latent frames, 1 440 000 samples per channel), where the
    fp32 oracle decoder would need ~4 TFLOP on the CPU: output length = hop * T, determinism, batch independence, and
    locality - the first 20 s of a 30 s decode equal a 20 s decode of the same latents away from the cut (the decoder's
    receptive field is finite, which is also why tiled and whole-sequence decode agree)."""
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    vcfg = ace355.VaeConfig()
    vae = NativeVae(vcfg, gpu_device)
    vae.load_state_dict(weightgen.make_vae_weights(vcfg.weight_shapes(), seed=4, mode="init"))
    g = torch.Generator().manual_seed(44)
    z = torch.randn(2, 64, 750, generator=g)
    w1 = vae.decode(z)
    w2 = vae.decode(z)
    assert w1.shape == (2, 2, vae.hop * 750) and torch.equal(w1, w2) and torch.isfinite(w1).all()
    solo = vae.decode(z[1:2])
    assert torch.equal(solo[0], w1[1]), "items of a batch are decoded independently"
    part = vae.decode(z[:, :, :500].contiguous())
    keep = vae.hop * (500 - 40)  # stay 40 latent frames away from the cut
    err = float((part[:, :, :keep] - w1[:, :, :keep]).abs().max())
    assert err <= 2e-3 * float(w1.abs().max()), err


@pytest.mark.parametrize("cfg_kw,B,frames", [
    (dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6)), 2, 40),
    (dict(), 1, 12),
    (dict(), 2, 7),
])
def test_encode_vs_oracle(gpu_device, cfg_kw, B, frames):
    """encoder half (strided convs as 2-tap convs over a shifted view, im2col'ed first conv, Gaussian head)
    against the (parity-unpinned) oracle restatement: mean, and the sampled latent with the oracle's own noise."""
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    from oracle import oobleck as o_vae
    cfg = ace355.VaeConfig(**cfg_kw)
    w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=2, mode="test")
    vae = NativeVae(cfg, gpu_device)
    vae.load_state_dict(w)
    L = cfg.hop * frames
    g = torch.Generator().manual_seed(frames)
    audio = 0.3 * torch.randn(B, 2, L, generator=g)
    o_cfg = o_vae.VaeConfig(**cfg_kw, encoder_hidden_size=cfg.encoder_hidden_size)
    mean_ref, std_ref = o_vae.encode_moments(o_cfg, w, audio)
    mean_emu, _ = o_vae.encode_moments(o_cfg, w, audio, emulate_bf16=True)
    mean = vae.encode(audio, sample=False)
    assert mean.shape == (B, 64, frames) == tuple(mean_ref.shape)
    snr_fp32, snr_emu, drift = _snr_db(mean, mean_ref), _snr_db(mean, mean_emu), _snr_db(mean_emu, mean_ref)
    print(f"vae encode {cfg_kw or 'full'} B={B} T={frames}: mean SNR vs fp32 oracle {snr_fp32:.1f} dB, vs bf16-storage oracle {snr_emu:.1f} dB "
          f"(oracle's own bf16 drift {drift:.1f} dB); latent rms {float(mean_ref.pow(2).mean().sqrt()):.3f}")
    assert snr_fp32 > drift - 6.0, (snr_fp32, drift)
    assert snr_emu > 30.0, snr_emu
    noise = torch.randn(B, 64, frames, generator=g)
    z = vae.encode(audio, noise=noise)
    z_ref = mean_ref + std_ref * noise
    assert _snr_db(z, z_ref) > min(snr_fp32, 40.0) - 3.0
    # round trip through the native decoder keeps the shape contract of the pair
    assert vae.decode(z).shape == (B, 2, L)


def test_encode_requires_encoder_weights(gpu_device):
    cfg, w, vae = _build(dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6)), gpu_device)
    with pytest.raises(RuntimeError, match="encoder"):
        vae.encode(torch.zeros(1, 2, cfg.hop * 4))


def test_encode_in_item_groups_under_a_small_budget(gpu_device):
    """The encoder shares the decode's activation budget: above it the batch runs in groups of items - exact, items are independent
    (the reference bounds encode memory by tiling, handler/vae_encode.py:47-86)."""
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae
    cfg = ace355.VaeConfig()
    w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=2, mode="test")
    audio = 0.3 * torch.randn(3, 2, cfg.hop * 20, generator=torch.Generator().manual_seed(5))
    outs = []
    for budget in (0, 3 * (cfg.hop * 20) * 128 * 2 * 3 // 2):   # default; then room for one item at a time
        vae = NativeVae(cfg, gpu_device)
        vae.load_state_dict(w)
        if budget:
            vae.set_decode_budget(budget)
        outs.append(vae.encode(audio, sample=False).cpu())
        vae.close()
    assert outs[0].shape == (3, 64, 20) and torch.equal(outs[0], outs[1])


def test_snake_placement_switch_agrees(gpu_device):
    """ACE355_VAE_EPISNAKE (csrc/vae.hip): 1 (default) applies the Snake of a tensor with one reader in its producer's epilogue (from the
    fp32 sum), 0 in the reader's window staging (from the stored bf16 tensor) - the same function with one rounding point fewer.  The
    switch is read once per process, so the other placement runs in a child process; both decodes and both encoder means must agree to
    the bf16-storage level (>= 35 dB) and differ (the switch really changes the path)."""
    import subprocess, sys, os, tempfile
    kw = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "import ace355\nfrom ace355 import weightgen\nfrom ace355.vae import NativeVae\n"
        "cfg = ace355.VaeConfig(**%r)\n"
        "w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=2, mode='test')\n"
        "vae = NativeVae(cfg, 'cuda:0'); vae.load_state_dict(w)\n"
        "z = torch.randn(2, 64, 37, generator=torch.Generator().manual_seed(5))\n"
        "a = 0.3 * torch.randn(2, 2, cfg.hop * 20, generator=torch.Generator().manual_seed(6))\n"
        "torch.save({'wav': vae.decode(z).cpu(), 'mean': vae.encode(a, sample=False).cpu()}, sys.argv[1])\n" % (root, kw))
    outs = {}
    with tempfile.TemporaryDirectory() as d:
        for v in ("0", "1"):
            path = os.path.join(d, f"o{v}.pt")
            env = dict(os.environ, ACE355_VAE_EPISNAKE=v)
            subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=600)
            outs[v] = torch.load(path)
    for k in ("wav", "mean"):
        snr = _snr_db(outs["1"][k], outs["0"][k])
        print(f"Snake placement 1 vs 0, {k}: {snr:.1f} dB")
        assert snr > 35.0, (k, snr)
        assert not torch.equal(outs["1"][k], outs["0"][k])


def test_fused_unit_forms_agree_bit_for_bit(gpu_device):
    """conv.hip runs the fused residual unit (C = 128) on a 4-wave 128-row tile (snake2(k7) through an LDS image) or, from ~1400 tiles up,
    on an 8-wave 256-row tile whose waves own 32 rows x all 128 channels (snake2(k7) from the accumulators straight into the k = 1
    stage's MFMAs).  `launch_conv` picks by problem size, and a windowed decode must equal a whole-sequence decode, so the two forms
    present the same K-slot order to the matrix unit (frag_kperm) and must give the SAME BITS.  ACE355_CONV_F8 = 0 / 1 forces one form at
    every size (read once per process: child processes); the full-width config so that the C = 128 units exist."""
    import subprocess, sys, os, tempfile
    import _vae_plan_cases as plan_cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the shapes below run the one-launch units on the 4-wave form by default: ACE355_CONV_F8=1 is what reaches the other one (each child
    # asserts the form of ITS process against the step lists it is about to execute)
    assert plan_cases.FUSED_FORM_CALLS == [(plan_cases.FULL, False, 2, 41), (plan_cases.FULL, True, 1, 12)]
    for kw, enc, B, fr in plan_cases.FUSED_FORM_CALLS:
        assert {plan_cases.form(st["plan"]) for st in plan_cases.vae_call(kw, enc, B, fr)["steps"] if st["fused"]} == {"w4"}
    code = (
        "import os, sys, torch; sys.path.insert(0, %r)\n"
        "import ace355\nfrom ace355 import native, weightgen\nfrom ace355.vae import NativeVae\n"
        "cfg = ace355.VaeConfig()\n"
        "want = {'bn': 128, 'tm': 256, 'ws': 1} if os.environ['ACE355_CONV_F8'] == '1' else {'bn': 128, 'tm': 128, 'ws': 0}\n"
        "for enc, B, T in ((False, 2, 41), (True, 1, cfg.hop * 12)):\n"
        "    fused = [st['plan'] for st in native.vae_plan(cfg, enc, B, T)['steps'] if st['fused']]\n"
        "    assert fused and all({k: p[k] for k in want} == want for p in fused), fused\n"
        "w = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=2, mode='test')\n"
        "vae = NativeVae(cfg, 'cuda:0'); vae.load_state_dict(w)\n"
        "z = torch.randn(2, 64, 41, generator=torch.Generator().manual_seed(5))\n"
        "a = 0.3 * torch.randn(1, 2, cfg.hop * 12, generator=torch.Generator().manual_seed(6))\n"
        "torch.save({'wav': vae.decode(z).cpu(), 'mean': vae.encode(a, sample=False).cpu()}, sys.argv[1])\n" % (root,))
    outs = {}
    with tempfile.TemporaryDirectory() as d:
        for v in ("0", "1"):
            path = os.path.join(d, f"o{v}.pt")
            env = dict(os.environ, ACE355_CONV_F8=v)
            subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=600)
            outs[v] = torch.load(path)
    for k in ("wav", "mean"):
        assert torch.isfinite(outs["1"][k]).all()
        assert torch.equal(outs["1"][k], outs["0"][k]), (k, float((outs["1"][k] - outs["0"][k]).abs().max()))
