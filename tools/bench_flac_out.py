#!/usr/bin/env python
"""FLAC output: the host encoder's path against the GPU frame encode (csrc/flac_out.hip), whole calls and pieces.

Rows: 1 x 30 s, 8 x 30 s, 8 x 240 s of stereo 48 kHz float32 in HBM, files on /dev/shm.  Columns: AudioSaver.save_paths with the flag off at
16 and at 2 host threads (the code every earlier commit has), with the flag on, and with the flag on and no MD5.  Before anything is timed
the flag-on files are compared with the flag-off files byte for byte.  Whole calls: wall clock around one synchronous call, 2 warm-up
rounds and then 7 rounds with the four columns interleaved, median [min - max].  Pieces of the GPU path, each timed on its own (device
events around batches of 10 for the kernels, wall clock for the host steps), so they do not sum to the call, where they overlap.

    python tools/bench_flac_out.py [--out profiles/flac_out_bench.txt] [--rows 1x30,8x30,8x240]
    python tools/bench_flac_out.py --encode-only 20 --rows 8x30     # only the three launches, for a kernel trace
"""
import argparse
import hashlib
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ace355 import native  # noqa: E402
from ace355.audio_out import AudioSaver, flac_encode_device, float_to_pcm16, normalize_audio_batch  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def signal(B, S, dev):
    """The signal of tests/perf/bench_audio_out.py: four harmonics under a slow envelope, a delayed right channel, a little noise."""
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.arange(S, device=dev) / 48000.0
    base = torch.stack([sum(torch.sin(2 * np.pi * (110.0 * (b + 1) * h) * t) / h for h in (1, 2, 3, 5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 0.25 * t))
                        for b in range(B)])
    wav = torch.stack([base, 0.7 * base.roll(7, dims=1)], dim=1) + 0.05 * torch.randn(B, 2, S, device=dev, generator=g)
    return normalize_audio_batch(wav, -1.0)[0]


def fmt(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f} - {max(v):.3f}]"


def events(fn, batches=5, per=10):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / per)
    return out


def wall(fn, n=7):
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def encode_call(pcm, sr=48000):
    B, S, Cn = pcm.shape
    p = native.flac_out_plan(B, S, Cn)
    scratch = torch.empty(p["scratch_bytes"], dtype=torch.uint8, device=pcm.device)
    out = torch.empty(p["out_bytes"], dtype=torch.uint8, device=pcm.device)
    rec = torch.empty(B, 4, dtype=torch.int64, device=pcm.device)

    def run():
        native.check(native.lib().ace355_flac_out_encode(native.ptr(pcm), B, S, Cn, sr, native.ptr(scratch), scratch.numel(), native.ptr(out), out.numel(),
                                                         native.ptr(rec), native.current_stream_ptr()), "flac_out_encode")
    return p, out, rec, run


def row(B, seconds, dev, out_dir, lines):
    S = int(seconds * 48000)
    wav = signal(B, S, dev)
    savers = {"off 16 thr": AudioSaver(n_threads=16, flac_on_gpu=False), "off 2 thr": AudioSaver(n_threads=2, flac_on_gpu=False),
              "gpu + md5": AudioSaver(n_threads=16, flac_on_gpu=True), "gpu no md5": AudioSaver(n_threads=16, flac_on_gpu=True, flac_md5=False)}
    paths = {k: [os.path.join(out_dir, f"{k.replace(' ', '_')}_{i}.flac") for i in range(B)] for k in savers}
    for k, s in savers.items():
        s.save_paths(wav, paths[k], 48000, "flac")
    want = [open(p, "rb").read() for p in paths["off 16 thr"]]
    assert [open(p, "rb").read() for p in paths["off 2 thr"]] == want
    assert [open(p, "rb").read() for p in paths["gpu + md5"]] == want, "the GPU path's files differ from the host encoder's"
    assert [open(p, "rb").read() for p in paths["gpu no md5"]] == [w[:26] + bytes(16) + w[42:] for w in want]
    assert savers["gpu + md5"].last_flac_report["path"] == "gpu" and savers["gpu no md5"].last_flac_report["path"] == "gpu"
    times = {k: [] for k in savers}
    for rnd in range(9):
        for k, s in savers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.save_paths(wav, paths[k], 48000, "flac")
            dt = (time.perf_counter() - t0) * 1e3
            if rnd >= 2:
                times[k].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    name = f"{B} x {seconds:g} s"
    lines.append(f"{name:<12}{sum(len(w) for w in want) / 1e6:9.2f}  " + "  ".join(f"{fmt(times[k]):>34}" for k in savers) +
                 f"  {med['off 16 thr'] / med['gpu + md5']:6.2f}x {med['off 2 thr'] / med['gpu + md5']:6.2f}x {med['off 16 thr'] / med['gpu no md5']:6.2f}x")
    # pieces
    pcm = float_to_pcm16(wav)
    p, out, rec, run = encode_call(pcm)
    t_inter = events(lambda: float_to_pcm16(wav))
    t_enc = events(run)
    torch.cuda.synchronize()
    r = rec.cpu().tolist()
    t_rec = wall(lambda: rec.cpu())
    host_out = torch.empty(p["out_bytes"], dtype=torch.uint8).pin_memory()
    host_pcm = torch.empty(pcm.numel(), dtype=torch.int16).pin_memory()

    def copy_frames():
        for i in range(B):
            at = i * p["item_stride"] + 42
            host_out[at:at + r[i][0]].copy_(out[at:at + r[i][0]], non_blocking=True)
    t_cf = wall(copy_frames)
    t_cp = wall(lambda: host_pcm.copy_(pcm.view(-1), non_blocking=True))
    one = host_pcm[:S * 2].numpy().tobytes()
    t_md5 = wall(lambda: hashlib.md5(one).digest(), 5)

    def write_files():
        for i, w in enumerate(want):
            with open(os.path.join(out_dir, f"w_{i}.flac"), "wb") as f:
                f.write(w)
    t_wr = wall(write_files)
    frame_bytes = sum(x[0] for x in r)
    model_ms = (pcm.numel() * 2 + 3 * frame_bytes) / HBM_BYTES_PER_S * 1e3
    lines.append(f"#   {name}: interleave {fmt(t_inter)} | three launches {fmt(t_enc)} | record read {fmt(t_rec)} | frame copies {fmt(t_cf)} | PCM copy {fmt(t_cp)}"
                 f" | MD5 of one item, one thread (hashlib) {fmt(t_md5)} | file writes, one thread {fmt(t_wr)}")
    lines.append(f"#   {name}: byte model (PCM read once, frame bytes written, read and written again, {HBM_BYTES_PER_S / 1e12:.1f} TB/s) {model_ms:.4f} ms;"
                 f" launches / model = {statistics.median(t_enc) / model_ms:.0f}x; MD5 share of the call (gpu + md5 minus gpu no md5) {med['gpu + md5'] - med['gpu no md5']:.3f} ms;"
                 f" units {p['units']}, scratch {p['scratch_bytes'] / 1e6:.1f} MB")
    assert flac_encode_device(pcm[:1], 48000)[0] == want[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1x30,8x30,8x240")
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--encode-only", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [(int(a), float(b)) for a, b in (r.split("x") for r in args.rows.split(","))]
    if args.encode_only:
        for B, sec in rows:
            pcm = float_to_pcm16(signal(B, int(sec * 48000), dev))
            _p, _o, _r, run = encode_call(pcm)
            for _ in range(args.encode_only):
                run()
            torch.cuda.synchronize()
        return
    out_dir = tempfile.mkdtemp(dir=args.dir)
    cols = ("off 16 thr", "off 2 thr", "gpu + md5", "gpu no md5")
    lines = [f"# FLAC output: the host encoder's path vs the GPU frame encode, {torch.cuda.get_device_name(0)}",
             "# AudioSaver.save_paths of float32 [B, 2, S] in HBM to files on " + (args.dir or "the temp dir") + "; the flag-on files equal the flag-off files byte for byte (asserted first)",
             "# whole calls: wall clock, 2 warm-up rounds, then 7 rounds with the columns interleaved; ms per call: median [min - max]",
             "# pieces: each alone (kernels: device events around batches of 10; host steps: wall clock), so they do not sum to the call",
             "# host threads held: off = n_threads for the whole call; gpu + md5 = one per item while hashing, then up to 16 for the file writes; gpu no md5 = the file writes only",
             f"{'batch':<12}{'files MB':>9}  " + "  ".join(f"{c + ' ms':>34}" for c in cols) + "  off16/gpu off2/gpu off16/nomd5"]
    try:
        for B, sec in rows:
            row(B, sec, dev, out_dir, lines)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
