"""The audio input stage on the GPU (csrc/audio_in.hip through ace355.audio_in): exact tests first - the conversion rule, the channel
map, impulse responses that read every phase's taps back, lengths, the clamp, the peak, reproducibility - then the resampled waveform
against the fp64 restatement (tests/_audio_in_oracle.py) at twice the fp32 restatement's own distance from it, then the handler seam
end to end.  Small shapes: a few seconds in all."""
import math
import random

import numpy as np
import pytest
import torch

import _audio_in_oracle as O
import _drift

pytestmark = pytest.mark.gpu

FORMATS = ("u8", "s16", "s24", "s32", "f32")
RESAMPLED = (44100, 32000, 16000, 96000, 88200)
L0 = 3001


def _run(dev, raw, fmt, channels, sr, offset=0):
    """raw sample bytes behind ``offset`` bytes of filler -> (wav on the GPU, peak as a float), with the peak checked on the way."""
    from ace355 import audio_in
    frames = len(raw) // (channels * O.BYTES[fmt])
    buf = audio_in.upload(np.frombuffer(b"\xa5" * offset + raw, dtype=np.uint8), dev)
    wav, peak = audio_in.resample_payload(buf, offset, fmt, channels, frames, sr)
    assert wav.shape == (2, audio_in.output_frames(frames, sr)) and wav.dtype == torch.float32 and wav.device == buf.device
    m = wav.abs().max()
    assert torch.equal(peak.view(torch.int32), m.reshape(1).view(torch.int32)), "the peak is max|wav|, bit for bit"
    return wav, float(peak)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- exact: 48 kHz
@pytest.mark.parametrize("fmt", FORMATS)
def test_passthrough_is_the_conversion_rule(gpu_device, fmt):
    """48 kHz: the same kernel with the resample skipped - libsndfile's rule, the channel map and the clamp, bit for bit against
    torch on the CPU, for samples at byte offsets 44 and 46 (46: no 4-byte sample is dword aligned; no 3-byte one ever is)."""
    g = torch.Generator().manual_seed(FORMATS.index(fmt))
    for channels in (1, 2, 6):
        n = L0 * channels
        if fmt == "f32":
            x = torch.rand(n, generator=g) * 3.0 - 1.5          # a quarter of them beyond +-1
            x[:6] = torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, -0.0, 1e-30])
            raw = x.numpy().astype("<f4").tobytes()
        else:
            a = torch.randint(0, 256, (n * O.BYTES[fmt],), generator=g, dtype=torch.int32).numpy().astype(np.uint8)   # every bit pattern
            nb = O.BYTES[fmt]
            a[:nb], a[nb:2 * nb] = 0, 255                                              # (255 ...: -1 LSB, or full scale for u8)
            a[2 * nb:3 * nb] = [0] * (nb - 1) + [0x80]                                 # the most negative sample
            a[3 * nb:4 * nb] = [255] * (nb - 1) + [0x7F]                               # the most positive one: 2^31 - 1 rounds to 1.0 in fp32
            raw = a.tobytes()
        want = O.normalize_to_stereo_48k(O.pcm_to_float(raw, fmt).reshape(L0, channels).T.contiguous(), 48000, torch.float32)
        for offset in (44, 46):
            got, peak = _run(gpu_device, raw, fmt, channels, 48000, offset)
            assert torch.equal(_bits(got), _bits(want)), (fmt, channels, offset)
            assert peak == float(want.abs().max())
        if channels == 1:
            assert torch.equal(got[0], got[1])
        assert float(got.abs().max()) <= 1.0


# ---------------------------------------------------------------------------------------------------- exact: impulse responses
def _impulse_expectation(sr, L, positions, signs):
    """What a sum of unit impulses (at most one inside any output's K-tap reach) must give: per output frame j = b n + p the dense fp32
    table's tap k[p][pos - b o + width].  Returns (expected where the tap's window argument is unclamped else 0, the dense value, live)."""
    k64, raw, o, n, width = O.dense_table(sr)
    k32, live = k64.to(torch.float32), raw.abs() < 6
    S = math.ceil(n * L / o)
    j = torch.arange(S)
    b, p = j // n, j % n
    want, dense, alive = torch.zeros(S), torch.zeros(S), torch.zeros(S, dtype=torch.bool)
    for pos, sign in zip(positions, signs):
        i = pos - b * o + width
        ok = (i >= 0) & (i < k32.shape[1])
        ic = i.clamp(0, k32.shape[1] - 1)
        val, lv = k32[p, ic] * sign, live[p, ic] & ok
        assert not bool((alive & lv).any()), "test bug: two impulses inside one output's reach"
        want = torch.where(lv, val, want)
        dense = torch.where(ok & ~lv & (dense == 0), val, dense)
        alive |= lv
    return want, dense, alive


def _check_impulses(dev, sr, L, positions, fmt="f32"):
    signs = [1.0 if i % 2 == 0 else -1.0 for i in range(len(positions))]
    x = torch.zeros(2, L)
    for pos, s in zip(positions, signs):
        x[0, pos], x[1, pos] = s, -s
    raw = O.float_to_pcm(x.T.contiguous() * (1.0 if fmt == "f32" else 0.5), fmt)   # (+-0.5 is exact in every PCM format)
    got, _peak = _run(dev, raw, fmt, 2, sr)
    got = got.cpu() * (1.0 if fmt == "f32" else 2.0)
    want, dense, alive = _impulse_expectation(sr, L, positions, signs)
    assert int(alive.sum()) > 0
    for c, sgn in ((0, 1.0), (1, -1.0)):
        y = got[c] * sgn
        assert torch.equal(y[alive], want[alive]), (sr, L, positions, c, "a phase's taps differ from the table")
        # outside the live taps: exact zero, or a kept tap with a clamped argument (the table's own ~1e-33)
        rest = y[~alive]
        assert bool(((rest == 0) | (rest == dense[~alive])).all()) and float(rest.abs().sum()) < 1e-20, (sr, L, positions, c)
    return got


@pytest.mark.parametrize("sr", [44100, 96000])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_impulse_reads_back_every_phase(gpu_device, sr, where):
    """1.0 x k plus exact zeros is k: an off-by-one in first[p], width, the zero padding at either end or the last partial tile moves or
    changes a tap."""
    pos = {"first": 0, "last": L0 - 1, "middle": 1500}[where]
    _check_impulses(gpu_device, sr, L0, [pos])


@pytest.mark.parametrize("sr,L", [(11025, L0), (352800, 30011), (32000, L0), (16000, L0), (88200, L0)])
def test_impulses_on_the_other_paths(gpu_device, sr, L):
    """11025 Hz: 640 phases, the table is read from global memory; 352800 Hz: a 512-frame tile; the other rates of the parity test."""
    from ace355 import audio_in, native
    tab = audio_in.tap_table(sr)
    p = native.audio_in_plan("f32", 2, L, tab["o"], tab["n"], tab["K"], tab["width"])
    assert (p["table_in_lds"], p["tile"]) == {11025: (0, 1024), 352800: (1, 512)}.get(sr, (1, 1024))
    assert p["grid"] > 1
    reach = 2 * tab["width"] + tab["o"] + 1   # impulses this far apart never meet inside one output's taps
    _check_impulses(gpu_device, sr, L, list(range(0, L - 1 - reach, reach)) + [L - 1])


def test_impulse_train_over_one_second(gpu_device):
    """44100 frames: 47 tiles.  An impulse every 401 frames (further apart than an output's reach) crosses every tile boundary at a
    different phase; s16 input this time, so the staging converts."""
    got = _check_impulses(gpu_device, 44100, 44100, list(range(0, 44100, 401)), fmt="s16")
    assert got.shape == (2, 48000)


@pytest.mark.parametrize("sr", RESAMPLED + (48000,))
def test_output_length_and_short_clips(gpu_device, sr):
    o, n = O.ratio(sr)
    for L in (1, 5, 2940, 3001):
        got = _check_impulses(gpu_device, sr, L, [L - 1] if L <= 5 else [0, L - 1]) if sr != 48000 else \
            _run(gpu_device, O.float_to_pcm(torch.full((L, 2), 0.25), "s16"), "s16", 2, sr)[0]
        assert got.shape == (2, math.ceil(n * L / o)), (sr, L)


def test_clamp_peak_and_same_bits(gpu_device):
    """Values beyond +-1 come out as exactly +-1 (the clamp is in the store), the peak is that of the clamped result, and the same call
    gives the same bits."""
    L = L0
    x = torch.stack([torch.full((L,), 3.0), torch.full((L,), -3.0)])
    raw = x.T.contiguous().numpy().astype("<f4").tobytes()
    for sr in (44100, 96000, 48000):
        got, peak = _run(gpu_device, raw, "f32", 2, sr, offset=2)
        inner = slice(64, got.shape[1] - 64)
        assert bool((got[0, inner] == 1.0).all()) and bool((got[1, inner] == -1.0).all()) and peak == 1.0
        assert float(got.abs().max()) == 1.0
    g = torch.Generator().manual_seed(11)
    noise = O.float_to_pcm((0.4 * torch.randn(44100 * 2, generator=g)).clamp(-1, 1), "s16")
    a, pa = _run(gpu_device, noise, "s16", 2, 44100, offset=44)
    b, pb = _run(gpu_device, noise, "s16", 2, 44100, offset=44)
    assert torch.equal(_bits(a), _bits(b)) and pa == pb and a.shape == (2, 48000)
    quiet, pq = _run(gpu_device, bytes(4 * L), "s16", 2, 44100)
    assert pq == 0.0 and not bool(quiet.any())


def test_refusals_on_the_launch(gpu_device):
    from ace355 import audio_in
    buf = audio_in.upload(np.zeros(4000, dtype=np.uint8), gpu_device)
    with pytest.raises(RuntimeError, match="does not hold"):
        audio_in.resample_payload(buf, 44, "s16", 2, 1000, 44100)     # 44 + 4000 bytes asked of 4000
    with pytest.raises(NotImplementedError, match="47999"):
        audio_in.resample_payload(buf, 0, "s16", 2, 10, 47999)
    with pytest.raises(ValueError):
        audio_in.resample_payload(buf[:3998], 0, "s16", 2, 10, 44100)
    with pytest.raises(NotImplementedError):
        audio_in.load_stereo_48k(O.wav_bytes(bytes(64), "s16", 2, 44100, tag=2, bits=4), gpu_device)
    with pytest.raises(ValueError, match="no audio frames"):
        audio_in.load_stereo_48k(O.wav_bytes(b"", "s16", 2, 44100), gpu_device)
    with pytest.raises(OSError):
        audio_in.load_stereo_48k("/nonexistent/clip.wav", gpu_device)


def test_torch_library_op(gpu_device):
    """torch.ops.ace355.audio_in is the same call in op form."""
    from ace355 import audio_in, native, ops  # noqa: F401
    g = torch.Generator().manual_seed(2)
    raw = O.float_to_pcm((0.3 * torch.randn(L0 * 2, generator=g)).clamp(-1, 1), "s16")
    buf = audio_in.upload(np.frombuffer(b"\0" * 44 + raw, dtype=np.uint8), gpu_device)
    want, want_peak = audio_in.resample_payload(buf, 44, "s16", 2, L0, 44100)
    wav, peak = torch.ops.ace355.audio_in(buf, 44, native.PCM_FORMATS.index("s16"), 2, L0, 44100)
    assert torch.equal(_bits(wav), _bits(want)) and torch.equal(_bits(peak), _bits(want_peak)) and wav.shape == (2, 3267)


# ---------------------------------------------------------------------------------------------------- tolerance
@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("sr", RESAMPLED)
def test_resampled_waveform_vs_fp64(gpu_device, sr, fmt):
    """Relative L2 against the fp64 restatement (fp64 taps, fp64 dense strided convolution, zero padded), per channel and over the whole
    tensor, gated at 2 x the distance of the fp32 restatement (the dense fp32 conv1d torchaudio executes) from fp64 in the same run.
    Why 2 x: a CPU emulation of the kernel's sparse, sequential fp32 sum sits at 1.02 - 1.15 x that drift (6.4e-8 .. 1.05e-7).
    Channel 0: a 1 kHz sine at 0.5; channel 1: N(0, 0.4^2) noise, which clamps ~0.4 % of the samples - the clamp is inside the gate.
    Measured on one MI355X: profiles/audio_in_parity.txt."""
    g = torch.Generator().manual_seed(sr)
    t = torch.arange(L0, dtype=torch.float64) / sr
    x = torch.stack([0.5 * torch.sin(2 * math.pi * 1000.0 * t), 0.4 * torch.randn(L0, generator=g, dtype=torch.float64)])
    raw = O.float_to_pcm(x.T.contiguous().clamp(-1, 1) if fmt == "s16" else x.T.contiguous(), fmt)
    xin = O.pcm_to_float(raw, fmt).reshape(L0, 2).T.contiguous()          # what the file holds: the input of all three
    ref64 = O.normalize_to_stereo_48k(xin, sr, torch.float64)
    ref32 = O.normalize_to_stereo_48k(xin, sr, torch.float32)
    got, _peak = _run(gpu_device, raw, fmt, 2, sr, offset=44)
    got = got.cpu()
    maxabs = float((got.double() - ref64).abs().max())
    print(f"audio_in parity {sr} {fmt}: max|gpu - ref64| {maxabs:.3e}, max|ref32 - ref64| {float((ref32.double() - ref64).abs().max()):.3e}, "
          f"clamped {float((ref64.abs() >= 1).double().mean()):.4f}")
    for name, sl in (("ch0", slice(0, 1)), ("ch1", slice(1, 2)), ("all", slice(0, 2))):
        measured, drift = _drift.rel(got[sl], ref64[sl]), _drift.rel(ref32[sl], ref64[sl])
        print(f"audio_in parity {sr} {fmt} {name}: gpu {measured:.3e} ref32 {drift:.3e} ratio {measured / drift:.3f}")
        _drift.check(f"audio_in {sr} Hz {fmt} {name}", measured, drift)


def test_against_torchaudio_when_present(gpu_device):
    """Optional: torchaudio's own Resample under the same gate.  Skips where torchaudio is absent (every machine this was built on);
    no required evidence rests on it."""
    ta = pytest.importorskip("torchaudio")
    g = torch.Generator().manual_seed(1)
    for sr in RESAMPLED:
        x = torch.stack([0.5 * torch.sin(2 * math.pi * 1000.0 * torch.arange(L0) / sr), 0.4 * torch.randn(L0, generator=g)]).float()
        theirs = torch.clamp(ta.transforms.Resample(sr, 48000)(x), -1.0, 1.0)
        ref64 = O.normalize_to_stereo_48k(x, sr, torch.float64)
        got, _ = _run(gpu_device, x.T.contiguous().numpy().astype("<f4").tobytes(), "f32", 2, sr)
        _drift.check(f"audio_in {sr} Hz vs torchaudio", _drift.rel(got.cpu(), theirs), max(_drift.rel(theirs, ref64), 1e-12))


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def clip_files(tmp_path_factory):
    """One second of 44.1 kHz stereo written by the package's own encoders, and a silent file."""
    from ace355.audio_out import flac_encode_pcm16, wav_encode
    d = tmp_path_factory.mktemp("audio_in")
    g = torch.Generator().manual_seed(3)
    t = torch.arange(44100) / 44100.0
    x = torch.stack([0.5 * torch.sin(2 * math.pi * 440.0 * t), 0.2 * torch.randn(44100, generator=g)]).T.contiguous()
    pcm = torch.round(x * 32767).to(torch.int16).numpy()
    files = {"flac": d / "clip.flac", "wav": d / "clip.wav", "wav32": d / "clip32.wav", "silent": d / "silent.wav"}
    files["flac"].write_bytes(flac_encode_pcm16(pcm, 44100))
    files["wav"].write_bytes(wav_encode(pcm, 44100))
    files["wav32"].write_bytes(wav_encode(x.numpy(), 44100))
    files["silent"].write_bytes(wav_encode(np.zeros((4410, 2), dtype=np.int16), 44100))
    return {k: str(v) for k, v in files.items()}, pcm


def _handler(dev):
    from ace355.backend import NativeHandler
    h = NativeHandler()
    h.device = str(dev)
    h.use_native_audio_in = True
    return h


def test_handler_loaders_end_to_end(gpu_device, clip_files):
    from ace355 import audio_in
    files, pcm = clip_files
    h = _handler(gpu_device)
    want, peak = audio_in.load_stereo_48k(files["flac"], gpu_device)
    assert want.shape == (2, 48000) and want.is_cuda and 0.4 < peak <= 1.0
    ref64 = O.normalize_to_stereo_48k(torch.from_numpy(pcm.astype(np.float32) / 32768.0).T.contiguous(), 44100, torch.float64)
    assert _drift.rel(want.cpu(), ref64) < 1e-6
    for key in ("flac", "wav"):   # the same int16 samples in two containers
        for name in ("process_src_audio", "process_target_audio"):
            got = getattr(h, name)(files[key])
            assert got.device == want.device and torch.equal(_bits(got), _bits(want)), (key, name)
    w32, _ = audio_in.load_stereo_48k(files["wav32"], gpu_device)
    assert torch.equal(_bits(h.process_src_audio(files["wav32"])), _bits(w32)) and _drift.rel(w32.cpu(), want.cpu()) < 1e-3   # (16-bit rounding apart)
    with open(files["wav"], "rb") as f:
        assert torch.equal(_bits(audio_in.load_stereo_48k(f.read(), gpu_device)[0]), _bits(want))
    random.seed(7)
    cut = audio_in.reference_segments(want)
    random.seed(7)
    ref = h.process_reference_audio(files["flac"])
    assert ref.shape == (2, 30 * 48000) and ref.is_cuda and torch.equal(_bits(ref), _bits(cut))
    random.seed(7)
    assert torch.equal(_bits(O.reference_cut(want.cpu())), _bits(cut))
    assert h.process_reference_audio(files["silent"]) is None
    assert h.process_src_audio(files["silent"]).shape == (2, 4800)
    assert h.process_src_audio(None) is None and h.process_src_audio("/nonexistent/clip.wav") is None
    assert h.process_src_audio(O.wav_bytes(bytes(64), "s16", 2, 44100, tag=2, bits=4)) is None   # no host loader to fall back to


def test_tiled_encode_takes_the_tensor_where_it_is(gpu_device, clip_files):
    """With the tiny VAE of the VAE tests: tiled_encode(process_src_audio(...)) equals the encode of the same tensor passed directly."""
    import ace355
    from ace355 import weightgen
    files, _pcm = clip_files
    cfg = ace355.VaeConfig(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))
    h = _handler(gpu_device)
    h.vae_config = cfg
    h.vae_state_dict = weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=2, mode="test")
    assert h._init_native_vae()
    wav = h.process_src_audio(files["flac"])
    torch.manual_seed(5)
    z = h.tiled_encode(wav)
    torch.manual_seed(5)
    direct = h.native_vae.encode(wav.clone()[None])[0]
    assert z.shape == direct.shape == (64, 48000 // cfg.hop) and torch.equal(_bits(z), _bits(direct))
    assert bool(torch.isfinite(z).all())
    h.native_vae.close()
