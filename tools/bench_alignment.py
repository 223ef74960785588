#!/usr/bin/env python
"""Lyric alignment cost at full size (24 layers, hidden 2048, weightgen seed-4 weights), on one GPU.

For 30 / 120 / 240 s songs (T = 750 / 3000 / 6000 latent frames), L = 769 and 2304 encoder rows, timestamp (N = 1) and score (N = 2) rows,
with the reference's default (layer, head) pairs (acestep/handler.py:129), it prints three times, each the median of --reps synchronised
calls after warm-up:
  * maps:     ace355_dit_cross_attention_maps alone (condition slots already built; the forward stops after layer 6's maps);
  * align:    the whole ace355.align.lyric_attention (slot build, rows, maps, the handlers' bf16 layout);
  * forward:  one full ace355_dit_forward at the same N, T, L;
and the ratio maps / forward.
Usage: python tools/bench_alignment.py [--reps 10]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import ace355
    from ace355 import align, native, weightgen
    from ace355.dit import NativeDit
    dev = torch.device("cuda:0")
    cfg = ace355.DitConfig()
    dit = NativeDit(cfg, dev)
    for name, shape in cfg.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
        native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
    native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
    prs = align.pairs(align.DEFAULT_LAYERS_HEADS, cfg)
    print(f"# {torch.cuda.get_device_name(0)}; pairs {prs}; median of {args.reps} synchronised calls (ms)")
    print(f"{'song':>5} {'L':>5} {'kind':>9} {'N':>2} {'maps':>8} {'align':>8} {'forward':>8} {'maps/fwd':>8}")
    g = torch.Generator().manual_seed(0)
    for secs, T in ((30, 750), (120, 3000), (240, 6000)):
        for L in (769, 2304):
            pred = torch.randn(1, T, 64, generator=g).to(torch.bfloat16)
            enc = torch.randn(1, L, cfg.hidden_size, generator=g).to(torch.bfloat16)
            ctx = torch.cat([0.5 * torch.randn(1, T, 64, generator=g), torch.ones(1, T, 64)], -1).to(torch.bfloat16)
            for kind in ("timestamp", "score"):
                p = pred.to(dev)
                x, t = align.alignment_rows(p, align.noise_like(p, 42), 8, kind)
                N = x.shape[0]
                xf, cf, tl = x.float(), ctx.to(dev).float().expand(N, -1, -1).contiguous(), t.float().tolist()
                dit.set_condition(0, enc[0].to(dev))
                slots = [0] * N
                t_maps = median_ms(lambda: dit.cross_attention_maps(xf, cf, tl, tl, slots, prs), args.reps)
                t_fwd = median_ms(lambda: dit.forward(xf, cf, tl, tl, slots), args.reps)
                t_align = median_ms(lambda: align.lyric_attention(dit, pred, enc, ctx, 8, 42, None, kind, torch.bfloat16), args.reps)
                print(f"{secs:>4}s {L:>5} {kind:>9} {N:>2} {t_maps:8.2f} {t_align:8.2f} {t_fwd:8.2f} {t_maps / t_fwd:8.3f}", flush=True)
    dit.close()


if __name__ == "__main__":
    main()
