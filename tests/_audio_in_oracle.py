"""CPU restatement of what the reference's IoAudioMixin computes between a decoded file and tiled_encode (io_audio.py:18-37, :89-110),
for the tests of ace355.audio_in.  oracle/ is frozen, so it lives here.

* ``pcm_to_float``: libsndfile's PCM -> float rule on raw little-endian sample bytes.
* ``dense_table``: torchaudio's ``_get_sinc_resample_kernel`` (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) in fp64, line by
  line; its fp32 rounding is the table torchaudio's ``Resample`` holds.
* ``resample``: torchaudio's ``_apply_sinc_resample_kernel``: zero padding (width, width + o), a dense conv1d of stride o with one
  output channel per phase, phases interleaved, cut to ceil(n L / o) - in fp64 with the fp64 table (the reference point) or in fp32 with
  the fp32 table (what torchaudio executes; its distance from fp64 is the drift the GPU result is gated by).
* ``normalize_to_stereo_48k``: io_audio.py:18-37 around it; ``reference_cut``: io_audio.py:89-110.

torchaudio is not installed on the machines this was written on: the restatement follows its published source, not a run of it.
"""
import math
import random
import struct

import numpy as np
import torch

RATE = 48000
BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4}


def pcm_to_float(raw: bytes, fmt: str) -> torch.Tensor:
    """Interleaved little-endian samples -> fp32 [samples] by libsndfile's rule."""
    a = np.frombuffer(raw, dtype=np.uint8)
    if fmt == "u8":
        return (torch.from_numpy(a.astype(np.int32)) - 128).to(torch.float32) / 128.0
    if fmt == "s16":
        return torch.from_numpy(a.view("<i2").astype(np.int32)).to(torch.float32) / 32768.0
    if fmt == "s24":
        b = a.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return torch.from_numpy(v).to(torch.float32) / 8388608.0
    if fmt == "s32":
        return torch.from_numpy(a.view("<i4").copy()).to(torch.float32) / 2147483648.0   # int32 -> fp32 rounds to nearest even
    assert fmt == "f32"
    return torch.from_numpy(a.view("<f4").copy())


def float_to_pcm(x: torch.Tensor, fmt: str) -> bytes:
    """fp32 / fp64 values in [-1, 1) -> the bytes of their nearest samples (test input making; not a rule under test)."""
    x = x.detach().double().reshape(-1)
    if fmt == "f32":
        return x.to(torch.float32).numpy().astype("<f4").tobytes()
    bits = 8 * BYTES[fmt]
    v = torch.round(x * (1 << (bits - 1))).clamp(-(1 << (bits - 1)), (1 << (bits - 1)) - 1).to(torch.int64).numpy()
    if fmt == "u8":
        return (v + 128).astype(np.uint8).tobytes()
    if fmt == "s16":
        return v.astype("<i2").tobytes()
    if fmt == "s32":
        return v.astype("<i4").tobytes()
    u = (v & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def ratio(sr: int):
    g = math.gcd(int(sr), RATE)
    return int(sr) // g, RATE // g


def dense_table(sr: int):
    """(fp64 table [n, 2 width + o], fp64 window argument before the clamp [n, 2 width + o], o, n, width)."""
    orig_freq, new_freq = ratio(sr)
    lowpass_filter_width, rolloff = 6, 0.99
    base_freq = min(orig_freq, new_freq)
    base_freq *= rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
    idx = torch.arange(-width, width + orig_freq, dtype=torch.float64)[None, None] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=torch.float64)[:, None, None] / new_freq + idx
    t *= base_freq
    raw = t.clone()
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / orig_freq
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels[:, 0], raw[:, 0], orig_freq, new_freq, width


def resample(x: torch.Tensor, sr: int, dtype=torch.float64) -> torch.Tensor:
    """x [C, L] -> [C, ceil(n L / o)] in ``dtype`` (fp64: fp64 table; fp32: the table rounded to fp32, as torchaudio holds it)."""
    if int(sr) == RATE:
        return x.to(dtype)
    k, _raw, o, n, width = dense_table(sr)
    k = k.to(dtype)[:, None]                                   # [n, 1, 2 width + o]
    C, L = x.shape
    w = torch.nn.functional.pad(x.to(dtype), (width, width + o))
    y = torch.nn.functional.conv1d(w[:, None], k, stride=o)    # [C, n, frames]
    y = y.transpose(1, 2).reshape(C, -1)
    return y[..., :math.ceil(n * L / o)]


def normalize_to_stereo_48k(audio: torch.Tensor, sr: int, dtype=torch.float64) -> torch.Tensor:
    """io_audio.py:18-37 on audio [channels, samples]."""
    if audio.shape[0] == 1:
        audio = torch.cat([audio, audio], dim=0)
    audio = audio[:2]
    if sr != RATE:
        audio = resample(audio, sr, dtype)
    return torch.clamp(audio.to(dtype), -1.0, 1.0)


def reference_cut(audio: torch.Tensor) -> torch.Tensor:
    """io_audio.py:89-110, line by line."""
    target_frames = 30 * 48000
    segment_frames = 10 * 48000

    if audio.shape[-1] < target_frames:
        repeat_times = math.ceil(target_frames / audio.shape[-1])
        audio = audio.repeat(1, repeat_times)

    total_frames = audio.shape[-1]
    segment_size = total_frames // 3

    front_start = random.randint(0, max(0, segment_size - segment_frames))
    front_audio = audio[:, front_start:front_start + segment_frames]

    middle_start = segment_size + random.randint(0, max(0, segment_size - segment_frames))
    middle_audio = audio[:, middle_start:middle_start + segment_frames]

    back_start = 2 * segment_size + random.randint(0, max(0, (total_frames - 2 * segment_size) - segment_frames))
    back_audio = audio[:, back_start:back_start + segment_frames]

    return torch.cat([front_audio, middle_audio, back_audio], dim=-1)


def wav_bytes(raw: bytes, fmt: str, channels: int, sr: int, extensible: bool = False, pre_chunks=(), data_size=None, tag=None, bits=None,
              fmt_extra: bytes = b"") -> bytes:
    """A RIFF/WAVE file around ``raw``.  ``pre_chunks``: (id, body) pairs written between fmt and data (odd bodies get the pad byte);
    ``data_size``: the size the data chunk CLAIMS (default: its real size); ``tag`` / ``bits``: override what the format implies."""
    nbytes = BYTES[fmt]
    code = 3 if fmt == "f32" else 1
    bits = 8 * nbytes if bits is None else bits
    align = channels * nbytes
    if extensible:
        sub = struct.pack("<H", code if tag is None else tag) + bytes.fromhex("000000001000800000aa00389b71")
        body = struct.pack("<HHIIHH", 0xFFFE, channels, sr, sr * align, align, bits) + struct.pack("<HHI", 22, bits, 0) + sub
    else:
        body = struct.pack("<HHIIHH", code if tag is None else tag, channels, sr, sr * align, align, bits) + fmt_extra
    out = b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body
    for cid, cbody in pre_chunks:
        out += cid + struct.pack("<I", len(cbody)) + cbody + (b"\0" if len(cbody) & 1 else b"")
    out += b"data" + struct.pack("<I", len(raw) if data_size is None else data_size) + raw
    return b"RIFF" + struct.pack("<I", len(out)) + out
