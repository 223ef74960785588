#!/usr/bin/env python
"""The native audio input stage vs the fp32 host restatement of the reference's path (same clip, same machine, same run)
-> profiles/audio_in_bench.txt.

Clips: 30 s and 240 s of stereo, as 44.1 kHz PCM_16 and as 48 kHz float32 (a sine and noise; the work does not depend on the values).
The bytes are what sits in a WAV file behind its 44-byte header; parsing the header is not timed on either side.

Native (ace355.audio_in): ``upload`` (one host-to-device copy of the raw payload from pageable memory, as ``load_stereo_48k`` makes
it) + ``resample_payload`` (one kernel: convert, channel map, resample, clamp, peak).  Timed with the upload and without it (payload
already on the GPU), device events around batches of ``--calls`` calls, after a warm-up; the peak is not read back inside the window.

Host: what IoAudioMixin._normalize_audio_to_stereo_48k executes after the decode, restated (tests/_audio_in_oracle.py): int16 -> fp32,
torchaudio's dense strided fp32 conv1d with the fp32 table, clamp - on ``--threads`` host threads (16), followed by the
host-to-device copy the reference then needs for tiled_encode (timed apart: "host + H2D").  torchaudio is not installed here, so this
is the restatement's time, not torchaudio's.

Beside both: the byte model - payload read + 8 bytes per output frame written, over 6.3 TB/s - as the least time the kernel could take.

Usage:  python tools/bench_audio_in.py [--runs 9] [--calls 10] [--threads 16] [--out profiles/audio_in_bench.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ace355  # noqa: E402,F401
from ace355 import audio_in  # noqa: E402
import _audio_in_oracle as O  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # the README's figure
CLIPS = [(44100, "s16", 30), (44100, "s16", 240), (48000, "f32", 30), (48000, "f32", 240)]


def make_clip(sr, fmt, seconds):
    L = sr * seconds
    g = torch.Generator().manual_seed(seconds)
    x = torch.stack([0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(L, dtype=torch.float64) / sr).float(), 0.3 * torch.randn(L, generator=g)])
    return np.frombuffer(O.float_to_pcm(x.T.contiguous().clamp(-1, 1), fmt), dtype=np.uint8), L


def batch_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def host_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def cell(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f} - {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9, help="timed batches per row and side")
    ap.add_argument("--calls", type=int, default=10, help="native calls per timed batch")
    ap.add_argument("--host-calls", type=int, default=2, help="host calls per timed batch")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_in_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_in.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.set_num_threads(args.threads)
    lines = [f"# native audio input stage vs the fp32 host restatement, {torch.cuda.get_device_name(dev)}, host restatement on {args.threads} threads",
             f"# {args.warmup} warm-up batches per side, then interleaved; native: device events around batches of {args.calls} calls; host: wall clock around",
             f"# batches of {args.host_calls} calls ending in a device synchronise; {args.runs} batches; ms per call: median [min - max]",
             "# model = (payload bytes + 8 bytes per output frame) / 6.3 TB/s: the least the kernel could take; GB/s = those bytes over the kernel's median",
             "# host = int16 / float -> fp32, dense strided fp32 conv1d (the restatement of torchaudio's Resample), clamp; + H2D = the copy tiled_encode then needs",
             f"{'clip':<22} {'payload MB':>10} {'out MB':>7} {'kernel ms':>28} {'upload + kernel ms':>28} {'host ms':>30} {'host + H2D ms':>30} {'model ms':>9} {'GB/s':>7} "
             f"{'host+H2D / native':>17}"]
    notes = []
    with torch.inference_mode():
        for sr, fmt, seconds in CLIPS:
            payload, L = make_clip(sr, fmt, seconds)
            S = audio_in.output_frames(L, sr)
            buf = audio_in.upload(payload, dev)
            xin = O.pcm_to_float(payload.tobytes(), fmt).reshape(L, 2) if fmt == "f32" else None
            pcm = torch.from_numpy(payload.view("<i2").reshape(L, 2).copy()) if fmt == "s16" else None

            def native_kernel():
                audio_in.resample_payload(buf, 0, fmt, 2, L, sr)

            def native_full():
                audio_in.resample_payload(audio_in.upload(payload, dev), 0, fmt, 2, L, sr)

            def host():
                x = (pcm.to(torch.float32) / 32768.0).T if fmt == "s16" else xin.T
                return O.normalize_to_stereo_48k(x.contiguous(), sr, torch.float32)

            def host_h2d():
                return host().to(dev)
            for _ in range(args.warmup):
                batch_ms(native_kernel, args.calls), batch_ms(native_full, args.calls), host_ms(host, 1), host_ms(host_h2d, 1)
            tk, tf, th, thd = [], [], [], []
            for _ in range(args.runs):
                tk.append(batch_ms(native_kernel, args.calls))
                tf.append(batch_ms(native_full, args.calls))
                th.append(host_ms(host, args.host_calls))
                thd.append(host_ms(host_h2d, args.host_calls))
            # the two sides computed the same thing
            got = audio_in.resample_payload(buf, 0, fmt, 2, L, sr)[0].cpu()
            rel = float((got.double() - host().double()).norm() / got.double().norm())
            nbytes = payload.size + 8 * S
            model = nbytes / HBM_BYTES_PER_S * 1e3
            mk, mf, mh = statistics.median(tk), statistics.median(tf), statistics.median(thd)
            lines.append(f"{f'{seconds} s {sr} Hz {fmt}':<22} {payload.size / 1e6:>10.2f} {8 * S / 1e6:>7.2f} {cell(tk):>28} {cell(tf):>28} {cell(th):>30} {cell(thd):>30} "
                         f"{model:>9.4f} {nbytes / (mk * 1e-3) / 1e9:>7.1f} {mh / mf:>16.1f}x")
            print(lines[-1], flush=True)
            notes.append(f"#   {seconds} s {sr} Hz {fmt}: the upload is {100 * (mf - mk) / mf:.0f} % of upload + kernel; kernel / model = {mk / model:.1f}; "
                         f"native vs host result, relative L2 {rel:.2e}")
            del buf, got
            torch.cuda.empty_cache()
    lines.append("# what bounds the call:")
    lines += notes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
