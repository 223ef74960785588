#!/usr/bin/env python
"""The bits the native VAE computes, as SHA-256 lines: run it on two builds and compare the outputs line for line.

Only the public Python API is used (NativeVae.decode / encode / stages / set_decode_budget), so the same file runs on any build.
Weights and inputs are seeded and generated on the CPU.  Cases:

  * small configuration (widths 256 / 128 / 64, ratios 6 / 4 / 2): decode B = 2, T = 37; encoder mean of B = 2, 23 frames; the public
    stage lists of both halves; one decode of B = 2, T = 200 split under a quarter of its whole-sequence budget
  * default configuration: decode B = 1, T = 24 and B = 2, T = 41; encoder mean of 12 frames; the stage lists
each under the default switches and under ACE355_VAE_EPISNAKE=0, ACE355_CONV_FUSE_RU=0, ACE355_CONV_F8=1, ACE355_CONV_TM=128 and
ACE355_CONV_RAS=0 - one child process per setting, the switches are read once.
Usage: python tools/vae_bits.py [--out FILE] [--root DIR]     (DIR: the checkout to import, default this file's)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

SETTINGS = [{}, {"ACE355_VAE_EPISNAKE": "0"}, {"ACE355_CONV_FUSE_RU": "0"}, {"ACE355_CONV_F8": "1"}, {"ACE355_CONV_TM": "128"}, {"ACE355_CONV_RAS": "0"}]
SMALL = dict(decoder_channels=64, channel_multiples=(1, 2, 4), downsampling_ratios=(2, 4, 6))


def child(root):
    sys.path.insert(0, root)
    import torch
    import ace355
    from ace355 import weightgen
    from ace355.vae import NativeVae

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.int32).numpy().tobytes()).hexdigest()

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    for name, kw, decodes, frames in (("small", SMALL, [(2, 37)], (2, 23)), ("default", dict(), [(1, 24), (2, 41)], (1, 12))):
        cfg = ace355.VaeConfig(**kw)
        vae = NativeVae(cfg, "cuda:0")
        vae.load_state_dict(weightgen.make_vae_weights({**cfg.weight_shapes(), **cfg.encoder_weight_shapes()}, seed=3, mode="test"))
        for B, T in decodes:
            print(f"{name} decode B={B} T={T} {sha(vae.decode(rnd(100 + T, B, 64, T)))}")
            print(f"{name} decoder stages T={T} {hashlib.sha256(json.dumps(vae.stages(False, T), sort_keys=True).encode()).hexdigest()}")
        B, n = frames
        audio = 0.3 * rnd(200 + n, B, 2, cfg.hop * n)
        print(f"{name} encode mean B={B} frames={n} {sha(vae.encode(audio, sample=False))}")
        print(f"{name} encoder stages L={cfg.hop * n} {hashlib.sha256(json.dumps(vae.stages(True, cfg.hop * n), sort_keys=True).encode()).hexdigest()}")
        if kw:
            z = rnd(300, 2, 64, 200)
            whole = vae.decode(z)
            vae.set_decode_budget(vae.decode_plan(2, 200)["activation_bytes"] // 4)
            plan = vae.decode_plan(2, 200)
            split = vae.decode(z)
            print(f"{name} decode B=2 T=200 split {plan['items_per_window']} x {plan['core_frames']} + {plan['overlap_frames']} {sha(split)} "
                  f"whole {sha(whole)}")
        vae.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.root)
    lines = []
    for env in SETTINGS:
        tag = " ".join(f"{k}={v}" for k, v in env.items()) or "defaults"
        clean = {k: v for k, v in os.environ.items() if not k.startswith("ACE355_")}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", args.root], env={**clean, **env}, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"[{tag}] failed with status {r.returncode}:\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            print(f"[{tag}] {ln}", flush=True)
            lines.append(f"[{tag}] {ln}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
