#!/usr/bin/env python
"""FLAC input, equality record -> profiles/flac_in_parity.txt.

Every stream of tests/_flac_streams.py is decoded on the GPU (ace355.audio_in.decode_flac) and compared, integer for integer, with the
oracle reader's samples (oracle.audio_out.flac_decode); then the stand-alone host program (tests/flac_in_host.cpp: the same per-frame
routines, built with AddressSanitizer and UBSan) decodes the same streams and 2000 seeded corruptions of the small ones, and its
statistics are appended.  The tests assert all of this; this file only records the counts.

Usage:  python tools/flac_in_parity.py [--out profiles/flac_in_parity.txt]
"""
from __future__ import annotations

import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ace355  # noqa: E402,F401
from ace355 import audio_in  # noqa: E402
import _flac_streams as S  # noqa: E402
import test_flac_in_cpu as T  # noqa: E402  (the case-file writer of the CPU test)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_in_parity.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flac_in_parity.py records a GPU run; none is visible")
    dev = torch.device("cuda:0")
    lines = [f"# FLAC frames decoded on the GPU vs the oracle reader, {torch.cuda.get_device_name(dev)}: decoded integers, no tolerance",
             f"{'stream':<24} {'bits':>4} {'ch':>2} {'frames':>6} {'samples':>8} {'path':>5} {'differing samples':>17}  note"]
    total = wrong = 0
    for name in S.STREAMS:
        data, rep, pcm, info = S.stream(name)
        buf, pinfo, report = audio_in.decode_flac(data, dev)
        raw = buf.cpu().numpy()
        got = raw.view("<i2").astype(np.int64) if pinfo.format == "s16" else raw.view("<i4").astype(np.int64) >> (32 - info["bps"])
        diff = int((got[:pcm.size].reshape(pcm.shape) != pcm).sum())
        total, wrong = total + pcm.size, wrong + diff
        note = f"fallback: {report['reason']}" if report["path"] == "host" else (f"max |sum coef x sample| = {rep['max_pred_sum']}" if rep["max_pred_sum"] else "")
        lines.append(f"{name:<24} {info['bps']:>4} {info['channels']:>2} {len(rep['blocks']):>6} {len(pcm):>8} {report['path']:>5} {diff:>17}  {note}")
    lines.append(f"# {len(S.STREAMS)} streams, {total} samples compared, {wrong} differ")
    cxx = shutil.which("g++") or shutil.which("clang++")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "flac_in_host")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "flac_in_host.cpp"), "-o", exe], check=True)
        files = {}
        for name in S.STREAMS:
            files[name] = os.path.join(tmp, f"{name}.case")
            T._case_file(files[name], name)
        r = subprocess.run([exe, "decode"] + [files[n] for n in S.STREAMS if n != "fake_header"], capture_output=True, text=True, check=True)
        lines.append(f"# the same routines on the CPU under AddressSanitizer + UBSan (tests/flac_in_host.cpp): {r.stdout.count(': equal')} streams equal, stderr empty: {not r.stderr}")
        r = subprocess.run([exe, "corrupt", "2000", "1"] + [files[n] for n in S.SMALL if n != "fake_header"], capture_output=True, text=True, check=True)
        lines.append("# " + r.stdout.strip() + f"; stderr empty: {not r.stderr}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
