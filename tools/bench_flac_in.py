#!/usr/bin/env python
"""FLAC input: the host decoder's path against the GPU frame decode (same clip, same process, interleaved rounds)
-> profiles/flac_in_bench.txt.

Clips: 30 s and 240 s of 44.1 kHz stereo (a sine and noise).  At 16 bits the file is the package's own encoder's (fixed predictors,
4096-sample blocks).  At 24 bits a numpy writer in this file makes it (fixed order 2, one Rice2 parameter per subframe, independent
channels, 4096-sample blocks): the host path does not read such a file, so only the new path's rows exist for it.  ``--file PATH``
times a file from elsewhere (a libFLAC one, say) the same way.  Neither writer emits LPC subframes: the restore pass's LPC cost is
not measured here.

Rows, ms per call, median [min - max] over ``--runs`` interleaved rounds after ``--warmup``:
  host path      load_stereo_48k(data): host decode (all CRCs and the MD5) + upload of the PCM + the resample kernel + the peak read-back
  host decode    flac_decode_pcm16(data) alone
  gpu path       load_stereo_48k(data, flac_on_gpu=True): index + upload of the file + decode launches + the resample kernel + one read-back
  index          ace355_flac_index alone (host)
  upload         the file's bytes to the GPU alone (device events around batches of ``--calls``)
  decode         the four decode launches alone on buffers already there (device events around batches of ``--calls``)
The host rows and the whole gpu path are wall clock around calls that end in a synchronise.  Beside them: the WAV call of the same
clip (upload + kernel) as profiles/audio_in_bench.txt has it.  The decoded payload is compared with the source samples before timing.

Usage:  python tools/bench_flac_in.py [--runs 7] [--calls 10] [--file PATH] [--out profiles/flac_in_bench.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from ace355 import audio_in, audio_out, native  # noqa: E402
import _flac_streams as S  # noqa: E402

BLOCK = 4096


def make_pcm(seconds: int, bps: int, sr: int = 44100) -> np.ndarray:
    L = sr * seconds
    g = torch.Generator().manual_seed(seconds)
    x = torch.stack([0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(L, dtype=torch.float64) / sr), 0.3 * torch.randn(L, generator=g).double()])
    return np.rint(x.T.clamp(-1, 1).numpy() * ((1 << (bps - 1)) - 1)).astype(np.int64)


def _crc16_rows(rows: np.ndarray) -> np.ndarray:
    """CRC-16 of every row of a uint8 matrix at once (one table step per column)."""
    tab = np.array(S._T16, dtype=np.uint32)
    c = np.zeros(len(rows), dtype=np.uint32)
    for j in range(rows.shape[1]):
        c = ((c << 8) & 0xFFFF) ^ tab[(c >> 8) ^ rows[:, j]]
    return c


def _subframe_bits(sig: np.ndarray, bps: int) -> np.ndarray:
    """One fixed order-2 subframe, partition order 0, one Rice parameter, as an array of bits (uint8 0 / 1)."""
    res = sig[2:] - 2 * sig[1:-1] + sig[:-2]
    u = np.where(res >= 0, 2 * res, -2 * res - 1)
    k = min(max(int(np.log2(max(float(u.mean()), 1.0))), 0), 30)   # Rice2: a 5-bit parameter
    q = u >> k
    head = [0] + [int(b) for b in format(8 | 2, "06b")] + [0]
    for v in sig[:2]:
        head += [int(b) for b in format(int(v) & ((1 << bps) - 1), f"0{bps}b")]
    head += [0, 1] + [0, 0, 0, 0] + [int(b) for b in format(k, "05b")]
    start = len(head) + np.concatenate([[0], np.cumsum(q + 1 + k)[:-1]])
    bits = np.zeros(len(head) + int((q + 1 + k).sum()), dtype=np.uint8)
    bits[:len(head)] = head
    bits[start + q] = 1
    for j in range(k):
        bits[start + q + 1 + j] = (u >> (k - 1 - j)) & 1
    return bits


def write_flac_numpy(pcm: np.ndarray, bps: int, sr: int = 44100) -> bytes:
    """A whole stream of BLOCK-sample frames, independent channels, fast enough for minutes of audio."""
    total, ch = pcm.shape
    frames = []
    for fno, at in enumerate(range(0, total, BLOCK)):
        x = pcm[at:at + BLOCK]
        head = S.frame_header(len(x), fno, ch - 1, bps, sr, False)
        bits = np.concatenate([np.frombuffer(head, dtype=np.uint8).repeat(8) >> np.tile(np.arange(7, -1, -1, dtype=np.uint8), len(head)) & 1] +
                              [_subframe_bits(x[:, c], bps) for c in range(ch)])
        frames.append(np.packbits(bits))
    crcs = {}
    for length in {len(f) for f in frames}:   # frames of one length share a vectorised CRC
        idx = [i for i, f in enumerate(frames) if len(f) == length]
        for i, c in zip(idx, _crc16_rows(np.stack([frames[i] for i in idx]))):
            crcs[i] = int(c)
    body = b"".join(f.tobytes() + crcs[i].to_bytes(2, "big") for i, f in enumerate(frames))
    si = S.BitWriter()
    si.put(BLOCK, 16), si.put(BLOCK, 16), si.put(0, 24), si.put(0, 24), si.put(sr, 20), si.put(ch - 1, 3), si.put(bps - 1, 5), si.put(total, 36)
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + si.tobytes() + bytes(16) + body


def wall_ms(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def cell(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f} - {max(xs):.3f}]" if xs else f"{'not read by the host path':>9}"


def wav_rows():
    """clip label -> 'upload + kernel ms' cell of profiles/audio_in_bench.txt."""
    out, path = {}, os.path.join(ROOT, "profiles", "audio_in_bench.txt")
    if os.path.exists(path):
        for line in open(path):
            if " s 44100 Hz s16" in line and not line.startswith("#"):
                parts = line.split("]")
                out[line.split(" s ")[0].strip()] = parts[1].strip() + "]"
    return out


def prepared_decode(data, dev):
    """The decode launches on buffers made once: () -> None, plus the payload they leave."""
    lib = native.lib()
    info, table = audio_in.flac_index(data)
    plan = native.FlacInPlanInfoC()
    native.check(lib.ace355_flac_in_plan(len(table), info.channels, info.bits_per_sample, info.max_block, info.total_samples, C.byref(plan)), "flac_in_plan")
    file_dev = audio_in.upload(np.frombuffer(data, dtype=np.uint8), dev)
    table_dev = torch.from_numpy(table).to(dev)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(plan.out_bytes, dtype=torch.uint8, device=dev)
    words = torch.empty(3, dtype=torch.int32, device=dev)
    stream = native.current_stream_ptr()

    def run():
        native.check(lib.ace355_flac_in_decode(C.byref(info), native.ptr(file_dev), len(data), native.ptr(table_dev), len(table), native.ptr(scratch),
                                               scratch.numel(), native.ptr(out), out.numel(), words.data_ptr() + 4, stream), "flac_in_decode")
    return run, out, words, plan, len(table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="calls per device-event batch (upload, decode)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=int, nargs="*", default=[30, 240])
    ap.add_argument("--file", default=None, help="also time this FLAC file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_in_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flac_in.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    clips = []
    for seconds in args.seconds:
        pcm16 = make_pcm(seconds, 16)
        clips.append((f"{seconds} s 44100 Hz 16 bit", audio_out.flac_encode_pcm16(pcm16.astype(np.int16), 44100), pcm16, 16, str(seconds)))
        pcm24 = make_pcm(seconds, 24)
        clips.append((f"{seconds} s 44100 Hz 24 bit", write_flac_numpy(pcm24, 24), pcm24, 24, None))
    if args.file:
        with open(args.file, "rb") as f:
            clips.append((os.path.basename(args.file), f.read(), None, None, None))
    wav = wav_rows()
    lines = [f"# FLAC input: the host decoder's path vs the GPU frame decode, {torch.cuda.get_device_name(dev)}",
             f"# {args.warmup} warm-up rounds, then {args.runs} interleaved rounds; host path, host decode, gpu path, index: wall clock around one call ending in a",
             f"# synchronise; upload, decode: device events around batches of {args.calls} calls; ms per call: median [min - max]",
             "# 16 bit: the package's encoder (fixed predictors, 4096-sample blocks); 24 bit: this tool's numpy writer (fixed order 2, one Rice2 parameter per",
             "# subframe); no LPC subframes in either, so the restore pass's LPC cost is not measured.  WAV call: upload + kernel of the same clip's PCM,",
             "# profiles/audio_in_bench.txt"]
    col = f"{'clip':<24} {'file MB':>8} {'frames':>7} {'lanes':>5} {'host path ms':>32} {'host decode ms':>32} {'gpu path ms':>28} {'index ms':>26} {'upload ms':>26} {'decode ms':>26} {'WAV call ms':>26} {'host / gpu':>10}"
    lines.append(col)
    notes = []
    with torch.inference_mode():
        for label, data, pcm, bps, wav_key in clips:
            run, out, words, plan, n_frames = prepared_decode(data, dev)
            run()
            st = words.cpu()[1:].tolist()
            assert st == [-1, 0], f"{label}: device status {st}"
            if pcm is not None:   # the decode computes the source samples
                raw = out.cpu().numpy()
                got = raw.view("<i2").astype(np.int64) if bps == 16 else raw.view("<i4").astype(np.int64) >> (32 - bps)
                assert np.array_equal(got[:pcm.size].reshape(pcm.shape), pcm), f"{label}: decoded samples differ from the source"
            host_ok = bps == 16 or (bps is None and audio_in.flac_index(data)[0].bits_per_sample <= 16)
            payload = np.frombuffer(data, dtype=np.uint8)
            fns = {"host path": (lambda: audio_in.load_stereo_48k(data, dev)) if host_ok else None,
                   "host decode": (lambda: audio_out.flac_decode_pcm16(data)) if host_ok else None,
                   "gpu path": lambda: audio_in.load_stereo_48k(data, dev, flac_on_gpu=True),
                   "index": lambda: audio_in.flac_index(data)}
            if host_ok:
                a, b = audio_in.load_stereo_48k(data, dev), audio_in.load_stereo_48k(data, dev, flac_on_gpu=True)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and a[1] == b[1], f"{label}: the two paths differ"
            t = {k: [] for k in list(fns) + ["upload", "decode"]}
            for r in range(args.warmup + args.runs):
                row = {k: wall_ms(f) for k, f in fns.items() if f is not None}
                row["upload"] = event_ms(lambda: audio_in.upload(payload, dev), args.calls)
                row["decode"] = event_ms(run, args.calls)
                if r >= args.warmup:
                    for k, v in row.items():
                        t[k].append(v)
            med = {k: statistics.median(v) for k, v in t.items() if v}
            ratio = f"{med['host path'] / med['gpu path']:9.1f}x" if host_ok else f"{'-':>10}"
            lines.append(f"{label:<24} {len(data) / 1e6:>8.2f} {n_frames:>7} {plan.entropy_lanes:>5} {cell(t['host path']):>32} {cell(t['host decode']):>32} {cell(t['gpu path']):>28} "
                         f"{cell(t['index']):>26} {cell(t['upload']):>26} {cell(t['decode']):>26} {wav.get(wav_key, 'not in that file'):>26} {ratio}")
            print(lines[-1], flush=True)
            parts = med["index"] + med["upload"] + med["decode"]
            notes.append(f"#   {label}: index + upload + decode = {parts:.3f} ms of the gpu path's {med['gpu path']:.3f} ms (the rest: allocations, the resample kernel, the read-back); "
                         f"decode per frame-lane round: {med['decode'] / plan.entropy_lanes:.3f} ms" + (f"; host decode is {100 * med['host decode'] / med['host path']:.0f} % of the host path" if host_ok else ""))
            del run, out, words
            torch.cuda.empty_cache()
    lines.append("# where the time goes:")
    lines += notes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
