"""Native input stage: file bytes -> fp32 ``[2, S]`` at 48 kHz, clamped to [-1, 1], on the GPU.

Reference: ``IoAudioMixin`` (acestep/core/generation/handler/io_audio.py:18-133): ``torchaudio.load`` / ``soundfile.read`` on the
host, ``_normalize_audio_to_stereo_48k`` (:18-37: mono duplicated, channels 0 and 1 kept, ``torchaudio.transforms.Resample(sr, 48000)``
on the CPU, clamp), ``is_silence`` and the 3 x 10 s cut of ``process_reference_audio`` (:89-110).  Here the host only finds the PCM
payload in the container and makes the resampler's tap table; the payload goes to the GPU as it sits in the file and one kernel
(csrc/audio_in.hip) converts, maps channels, resamples, clamps and leaves the peak.

* WAV: RIFF with ``fmt `` codes 1 (PCM 8 / 16 / 24 / 32 bit), 3 (IEEE float32) and 0xFFFE (extensible, those two sub-formats); unknown
  chunks are skipped, a ``data`` chunk that claims more than the file holds is cut at the end of the file (libsndfile does the same).
* FLAC: the package's own decoder (``audio_out.flac_decode_pcm16``: <= 16 bits, 1-2 channels), whose int16 frames are the payload.
  With ``flac_on_gpu`` the file goes up as it is instead and its frames are decoded on the GPU (``decode_flac``, csrc/flac_in.hip:
  16 to 24 bits, 1-2 channels); what the frame index refuses, or a frame the device rejects, goes back to the line above.
* Anything else - RF64, ADPCM, float64, mp3, deeper FLAC, a rate whose tap table the plan refuses - raises ``NotImplementedError``: the
  seam (``backend.NativeAudioInMixin``) hands those to the host's own method.

The resampler is restated from torchaudio's published definition (``sinc_interp_hann``, ``lowpass_filter_width = 6``,
``rolloff = 0.99``); torchaudio itself is on neither machine image this was built on, so parity with it is unpinned.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import random
import struct
import warnings
from typing import Dict, NamedTuple, Tuple, Union

import numpy as np
import torch

from . import native

TARGET_RATE = 48000
LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # bytes 2 .. 15 of KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT


class PcmInfo(NamedTuple):
    format: str        # native.PCM_FORMATS
    channels: int
    sample_rate: int
    frames: int
    offset: int        # byte offset of the payload in the buffer it was found in


# ---------------------------------------------------------------------------------------------------- containers
def parse_wav(data) -> PcmInfo:
    """Where the samples of a RIFF/WAVE file are and what they are.  ``data``: bytes-like.  ``NotImplementedError`` for everything this
    stage does not read."""
    mv = memoryview(data)
    size = len(mv)
    if size < 12 or bytes(mv[0:4]) != b"RIFF" or bytes(mv[8:12]) != b"WAVE":
        raise NotImplementedError("not a RIFF/WAVE file (RF64 and other containers stay with the host path)")
    pos, fmt = 12, None
    while pos + 8 <= size:
        cid, csize = bytes(mv[pos:pos + 4]), struct.unpack_from("<I", mv, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if csize < 16 or body + 16 > size:
                raise NotImplementedError("WAV: short fmt chunk")
            tag, channels, rate, _byte_rate, align, bits = struct.unpack_from("<HHIIHH", mv, body)
            if tag == 0xFFFE:
                if csize < 40 or body + 40 > size:
                    raise NotImplementedError("WAV: short extensible fmt chunk")
                sub = bytes(mv[body + 24:body + 40])
                if sub[2:] != _KSDATAFORMAT_TAIL:
                    raise NotImplementedError("WAV: unknown extensible sub-format")
                tag = struct.unpack_from("<H", sub, 0)[0]
            fmt = (tag, channels, rate, align, bits)
        elif cid == b"data":
            if fmt is None:
                raise NotImplementedError("WAV: data chunk ahead of fmt")
            tag, channels, rate, align, bits = fmt
            name = {(1, 8): "u8", (1, 16): "s16", (1, 24): "s24", (1, 32): "s32", (3, 32): "f32"}.get((tag, bits))
            if name is None:
                raise NotImplementedError(f"WAV: format tag {tag} with {bits} bits per sample is not read natively")
            if channels < 1:
                raise NotImplementedError("WAV: no channels")
            per_frame = channels * native.PCM_BYTES[native.PCM_FORMATS.index(name)]
            if align != per_frame:
                raise NotImplementedError(f"WAV: block align {align} is not channels x sample size ({per_frame})")
            return PcmInfo(name, channels, rate, min(csize, size - body) // per_frame, body)
        pos = body + csize + (csize & 1)
    raise NotImplementedError("WAV: no data chunk")


def _flac_payload(data) -> Tuple[np.ndarray, PcmInfo]:
    lib = native.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    frames, ch, sr, bps = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    native.check(lib.ace355_flac_info(buf.ctypes.data, buf.size, C.byref(frames), C.byref(ch), C.byref(sr), C.byref(bps)), "flac_info")
    if bps.value > 16 or ch.value > 2:
        raise NotImplementedError(f"FLAC with {bps.value} bits per sample / {ch.value} channels is not decoded natively (<= 16 bits, 1-2 channels)")
    from .audio_out import flac_decode_pcm16
    pcm, rate = flac_decode_pcm16(bytes(data))
    return pcm.reshape(-1).view(np.uint8), PcmInfo("s16", int(ch.value), int(rate), int(pcm.shape[0]), 0)


def flac_index(data) -> Tuple["native.FlacStreamInfoC", np.ndarray]:
    """``ace355_flac_index``: (STREAMINFO, the frame table int64 [frames, 4] = byte offset, byte length, first sample, block size) of a
    FLAC file's bytes.  ``NotImplementedError`` with the index's text for a stream it refuses."""
    lib = native.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    info, n, cap = native.FlacStreamInfoC(), C.c_int64(0), 4096
    for _attempt in range(2):
        table = np.empty((cap, 4), dtype=np.int64)
        if lib.ace355_flac_index(buf.ctypes.data, buf.size, C.byref(info), table.ctypes.data, cap, C.byref(n)) == native.OK:
            return info, table[:n.value]
        if n.value <= cap:
            break
        cap = int(n.value)
    raise NotImplementedError(native.last_error())


def _flac_host(data, device, report: Dict[str, object], reason: str) -> Tuple[torch.Tensor, PcmInfo, Dict[str, object]]:
    """The fallback of ``decode_flac``: the flag-off host path (``_flac_payload``), which is the authority - what it raises surfaces, with
    the report attached as ``flac_report``."""
    report.update(path="host", reason=reason)
    report.pop("words", None)
    try:
        payload, info = _flac_payload(data)
    except Exception as exc:
        exc.flac_report = report
        raise
    return upload(payload, device), info, report


def _flac_status(report: Dict[str, object], words) -> Union[str, None]:
    """Reads (first bad frame, code) out of the fetched status words into the report; the fallback's reason, or None when every frame
    decoded."""
    frame, code = int(words[1]), int(words[2])
    if frame < 0:
        return None
    report.update(frame=frame, code=code)
    return f"frame {frame}: {native.FLAC_STATUS[code] if 0 <= code < len(native.FLAC_STATUS) else code}"


def decode_flac(data, device, sync: bool = True) -> Tuple[torch.Tensor, PcmInfo, Dict[str, object]]:
    """A FLAC file's bytes -> (the uint8 device payload ``resample_payload`` takes, what is in it, a report).  The bytes are uploaded as
    they are, indexed by frame on the host and decoded on the GPU (16 to 24 bits, 1-2 channels; int16 at 16 bits, left-justified int32
    above); every frame's CRC-16 is checked there, the STREAMINFO MD5 is not.  ``report["path"]`` is ``"gpu"`` or ``"host"``; after a
    fallback ``report["reason"]`` holds the index's refusal or the device status (``report["frame"]``, ``report["code"]``:
    ``native.FLAC_STATUS``), and the payload is the host decoder's - at more than 16 bits there is none and the ``NotImplementedError``
    of the host path is raised.  ``sync=False`` leaves the status unread in ``report["words"]`` (int32 [3] on the device: a slot for
    the resampler's peak, then first bad frame and code) for a caller that fetches it with its own synchronisation."""
    device = torch.device(device)
    if device.type != "cuda":
        raise NotImplementedError("the native audio input stage runs on the GPU (no CPU fallback)")
    report: Dict[str, object] = {"path": "gpu", "reason": None, "frame": None, "code": None}
    lib = native.lib()
    try:
        info, table = flac_index(data)
    except NotImplementedError as exc:
        return _flac_host(data, device, report, str(exc))
    plan = native.FlacInPlanInfoC()
    if lib.ace355_flac_in_plan(len(table), info.channels, info.bits_per_sample, info.max_block, info.total_samples, C.byref(plan)) != native.OK:
        return _flac_host(data, device, report, native.last_error())
    report["frames"] = len(table)
    file_dev = upload(np.frombuffer(data, dtype=np.uint8), device)
    table_dev = torch.from_numpy(table).to(device)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=device)
    out = torch.empty(plan.out_bytes, dtype=torch.uint8, device=device)
    words = torch.empty(3, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        native.check(lib.ace355_flac_in_decode(C.byref(info), native.ptr(file_dev), len(memoryview(data)), native.ptr(table_dev), len(table),
                                               native.ptr(scratch), scratch.numel(), native.ptr(out), out.numel(), words.data_ptr() + 4,
                                               native.current_stream_ptr()), "flac_in_decode")
    pcm = PcmInfo(native.PCM_FORMATS[plan.out_format], int(info.channels), int(info.sample_rate), int(info.total_samples), 0)
    if not sync:
        report["words"] = words
        return out, pcm, report
    reason = _flac_status(report, words.cpu())
    if reason is not None:
        return _flac_host(data, device, report, reason)
    return out, pcm, report


def find_payload(data) -> Tuple[np.ndarray, PcmInfo]:
    """(the bytes that go to the GPU as a uint8 array, where and what the samples in them are)."""
    head = bytes(memoryview(data)[0:4])
    if head == b"fLaC":
        return _flac_payload(data)
    if head == b"RIFF":
        return np.frombuffer(data, dtype=np.uint8), parse_wav(data)
    raise NotImplementedError("neither RIFF/WAVE nor FLAC: the host path reads this file")


# ---------------------------------------------------------------------------------------------------- tap table
def rate_ratio(sample_rate: int) -> Tuple[int, int, int]:
    """(o, n, width) of torchaudio's resampler from ``sample_rate`` to 48 kHz; width 0 at 48 kHz, where there is no table."""
    sample_rate = int(sample_rate)
    if sample_rate <= 0:
        raise NotImplementedError(f"sample rate {sample_rate}")
    g = math.gcd(sample_rate, TARGET_RATE)
    o, n = sample_rate // g, TARGET_RATE // g
    if o == n:
        return 1, 1, 0
    base = min(o, n) * ROLLOFF
    return o, n, math.ceil(LOWPASS_FILTER_WIDTH * o / base)


def dense_taps(sample_rate: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """torchaudio's ``_get_sinc_resample_kernel`` for (sample_rate -> 48000), operation for operation in fp64: the table
    [n, 2 width + o] before its rounding to fp32, and which of its taps have an unclamped window argument."""
    o, n, width = rate_ratio(sample_rate)
    base = min(o, n) * ROLLOFF
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = t * base
    live = t.abs() < LOWPASS_FILTER_WIDTH
    t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels = kernels * (window * scale)
    return kernels, live


def tap_table(sample_rate: int) -> Dict[str, object]:
    """The compacted table of a rate on the host: ``first`` int32 [n], ``taps`` fp32 [n, K] (the dense fp32 table's entries
    [first[p], first[p] + K) of phase p), with o, n, K, width.  K is the largest number of unclamped taps of any phase; the taps left out
    have a clamped window argument (~1e-33).  Rates whose dense table exceeds the plan's cap raise ``NotImplementedError``."""
    o, n, width = rate_ratio(sample_rate)
    if o == n:
        return {"o": 1, "n": 1, "K": 0, "width": 0, "first": None, "taps": None}
    dense = 2 * width + o
    if n * dense > native.AUDIO_IN_MAX_DENSE_TAPS:
        raise NotImplementedError(f"the tap table of {sample_rate} Hz has {n} x {dense} taps; the native stage stops at {native.AUDIO_IN_MAX_DENSE_TAPS}")
    k64, live = dense_taps(sample_rate)
    k32 = k64.to(torch.float32)
    count = live.sum(dim=1)
    K = int(count.max())
    lo = live.to(torch.int8).argmax(dim=1)                   # the first live tap of each phase (the live taps are consecutive)
    first = torch.minimum(lo, torch.full_like(lo, dense - K))
    cols = first[:, None] + torch.arange(K)[None]
    return {"o": o, "n": n, "K": K, "width": width, "first": first.to(torch.int32).contiguous(), "taps": k32.gather(1, cols).contiguous()}


_TABLES: Dict[Tuple[int, str], Dict[str, object]] = {}


def device_table(sample_rate: int, device) -> Dict[str, object]:
    """``tap_table`` with ``first`` / ``taps`` on ``device``, made once per (rate, device)."""
    key = (int(sample_rate), str(torch.device(device)))
    tab = _TABLES.get(key)
    if tab is None:
        tab = dict(tap_table(sample_rate))
        if tab["K"]:
            tab["first"], tab["taps"] = tab["first"].to(device), tab["taps"].to(device)
        _TABLES[key] = tab
    return tab


def output_frames(frames: int, sample_rate: int) -> int:
    o, n, _w = rate_ratio(sample_rate)
    return -(-n * int(frames) // o)


# ---------------------------------------------------------------------------------------------------- the stage
def upload(payload: np.ndarray, device) -> torch.Tensor:
    """The payload bytes as a uint8 device tensor whose size is a multiple of 4 (the kernel loads dwords), zero padded."""
    n = int(payload.size)
    buf = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (a read-only buffer: it is only read)
        src = torch.from_numpy(payload)
    buf[:n].copy_(src)
    buf[n:].zero_()
    return buf


def resample_payload(buf: torch.Tensor, offset: int, format: str, channels: int, frames: int, sample_rate: int,
                     peak: Union[torch.Tensor, None] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ace355_audio_in_run``: ``buf`` uint8 on the GPU (size a multiple of 4) holding ``frames`` x ``channels`` interleaved samples of
    ``format`` from byte ``offset`` -> (fp32 [2, S] at 48 kHz clamped to [-1, 1], its peak as a fp32 [1] tensor), both on ``buf``'s device.
    A request the plan refuses raises ``NotImplementedError`` with the plan's text.  ``peak``: a fp32 [1] tensor on that device to leave
    the peak in (a new one otherwise)."""
    if not (buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() % 4 == 0):
        raise ValueError("resample_payload: a contiguous uint8 CUDA tensor with a multiple of 4 bytes")
    tab = device_table(sample_rate, buf.device)
    rq = native.audio_in_request(format, channels, frames, tab["o"], tab["n"], tab["K"], tab["width"])
    info = native.AudioInPlanInfoC()
    lib = native.lib()
    if lib.ace355_audio_in_plan(C.byref(rq), C.byref(info)) != native.OK:
        raise NotImplementedError(native.last_error())
    out = torch.empty(2, info.out_frames, dtype=torch.float32, device=buf.device)
    if peak is None:
        peak = torch.empty(1, dtype=torch.float32, device=buf.device)
    with torch.cuda.device(buf.device):
        native.check(lib.ace355_audio_in_run(C.byref(rq), native.ptr(buf), buf.numel(), int(offset), native.ptr(tab["first"]), native.ptr(tab["taps"]),
                                             native.ptr(out), native.ptr(peak), native.current_stream_ptr()), "audio_in_run")
    return out, peak


def _load_flac_on_gpu(data, device) -> Tuple[torch.Tensor, float]:
    """``load_stereo_48k`` of a FLAC file through ``decode_flac``: the resampler is enqueued on the decoded payload whatever the decode
    will report, and its peak and the decode's status come back in one copy - the only synchronisation of the call.  A bad status
    discards the result and the host decoder's payload takes the same road."""
    buf, info, report = decode_flac(data, device, sync=False)
    if report["path"] == "gpu":
        words = report.pop("words")
        wav, _peak = resample_payload(buf, 0, info.format, info.channels, info.frames, info.sample_rate, peak=words[0:1].view(torch.float32))
        host = words.cpu()
        reason = _flac_status(report, host)
        if reason is None:
            return wav, float(host[0:1].view(torch.float32).item())
        buf, info, report = _flac_host(data, device, report, reason)
    if info.frames < 1:
        raise ValueError("the file holds no audio frames")
    wav, peak = resample_payload(buf, info.offset, info.format, info.channels, info.frames, info.sample_rate)
    return wav, float(peak.item())


def load_stereo_48k(path_or_bytes: Union[str, os.PathLike, bytes, bytearray, memoryview], device, flac_on_gpu: bool = False) -> Tuple[torch.Tensor, float]:
    """A WAV or FLAC file (path or contents) -> (wav fp32 [2, S] at 48 kHz on ``device``, clamped to [-1, 1]; max|wav|): what
    ``torchaudio.load`` + ``_normalize_audio_to_stereo_48k`` return (io_audio.py:18-37, :78, :129).  ``OSError`` for an unreadable path,
    ``ValueError`` for a file without frames, ``NotImplementedError`` for what this stage does not read.  ``flac_on_gpu``: a FLAC file's
    frames are decoded on the GPU (``decode_flac``) instead of by the host decoder; every other file is read as without it."""
    device = torch.device(device)
    if device.type != "cuda":
        raise NotImplementedError("the native audio input stage runs on the GPU (no CPU fallback)")
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = path_or_bytes
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    if flac_on_gpu and bytes(memoryview(data)[0:4]) == b"fLaC":
        return _load_flac_on_gpu(data, device)
    payload, info = find_payload(data)
    if info.frames < 1:
        raise ValueError("the file holds no audio frames")
    device_table(info.sample_rate, device)   # (a rate the stage refuses raises here, before anything is uploaded)
    wav, peak = resample_payload(upload(payload, device), info.offset, info.format, info.channels, info.frames, info.sample_rate)
    return wav, float(peak.item())


def reference_segments(wav: torch.Tensor) -> torch.Tensor:
    """The cut of ``process_reference_audio`` (io_audio.py:89-110) on ``wav`` [2, S], wherever it lives: repeat up to 30 s, then three
    10 s segments from the front, middle and back third, their starts drawn by three calls of Python's global ``random.randint`` in the
    reference's order and with its bounds - the same ``random.seed`` gives the same starts."""
    target_frames = 30 * TARGET_RATE
    segment_frames = 10 * TARGET_RATE
    if wav.shape[-1] < target_frames:
        wav = wav.repeat(1, math.ceil(target_frames / wav.shape[-1]))
    total_frames = wav.shape[-1]
    segment_size = total_frames // 3
    front_start = random.randint(0, max(0, segment_size - segment_frames))
    middle_start = segment_size + random.randint(0, max(0, segment_size - segment_frames))
    back_start = 2 * segment_size + random.randint(0, max(0, (total_frames - 2 * segment_size) - segment_frames))
    return torch.cat([wav[:, s:s + segment_frames] for s in (front_start, middle_start, back_start)], dim=-1)
