#!/usr/bin/env python
"""LoRA merge cost and per-request cost with an adapter, at full size (24 layers, hidden 2048), on one GPU.

Reports (one JSON line, plus readable lines):
  * merge ms (ace355_dit_set_adapters, host clock around a synchronised call; pristine copies already made) for the attention targets
    (self / cross q, k, v, o) at rank 8 and 64, and for all ten target kinds at rank 64 and 256;
  * the metric request's DiT part (8 songs x 30 s, 27 steps, CFG 7 + APG) with a rank-64 adapter on all ten kinds against no adapter,
    alternating in one process.
Usage: python tools/bench_lora.py [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ATTN = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
        "cross_attn.q_proj", "cross_attn.k_proj", "cross_attn.v_proj", "cross_attn.o_proj")
ALL = ATTN + ("mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit, generate_latents
    from ace355.lora import LoraTerm
    dev = torch.device("cuda:0")
    cfg = ace355.DitConfig()
    dit = NativeDit(cfg, dev)
    for name, shape in cfg.weight_shapes().items():
        wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
        native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
    native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
    shapes = cfg.weight_shapes()
    g = torch.Generator(device=dev).manual_seed(0)

    def terms(kinds, rank):
        out = []
        for li in range(cfg.num_hidden_layers):
            for k in kinds:
                name = f"layers.{li}.{k}.weight"
                o, i = shapes[name]
                out.append(LoraTerm(name, torch.randn(rank, i, device=dev, generator=g).to(torch.bfloat16),
                                    torch.randn(o, rank, device=dev, generator=g).to(torch.bfloat16), 1e-4))
        return out

    def merge_ms(ts):
        dit.set_adapters(ts)   # (first touch: pristine copies)
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dit.set_adapters(ts)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times), min(times)

    res = {}
    for label, kinds, rank in (("attn_r8", ATTN, 8), ("attn_r64", ATTN, 64), ("all10_r64", ALL, 64), ("all10_r256", ALL, 256)):
        ts = terms(kinds, rank)
        med, best = merge_ms(ts)
        weights = sum(shapes[t.name][0] * shapes[t.name][1] for t in ts)
        res[label] = {"median_ms": round(med, 3), "min_ms": round(best, 3), "weights": weights,
                      "hbm_GBps_at_median": round(4 * weights / med / 1e6, 1)}
        print(f"merge {label}: median {med:.3f} ms, min {best:.3f} ms ({weights / 1e9:.2f} G weights, read pristine + write live: "
              f"{4 * weights / med / 1e6:.0f} GB/s)", flush=True)
        dit.clear_adapters()

    # the metric request's DiT part, with and without a rank-64 adapter on all ten kinds, alternating
    gen = torch.Generator().manual_seed(0)
    B, T, L = 8, 750, 769
    enc = torch.randn(1, L, cfg.hidden_size, generator=gen).expand(B, -1, -1).contiguous().to(dev)
    ctx = torch.cat([0.5 * torch.randn(B, T, 64, generator=gen), torch.ones(B, T, 64)], -1).to(dev)
    null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=4)
    lora64 = terms(ALL, 64)
    kw = dict(seed=list(range(B)), infer_steps=27, diffusion_guidance_sale=7.0)

    def request():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        generate_latents(dit, null, enc, ctx, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    for mode in ("none", "r64"):   # warm-up of both states
        dit.set_adapters(lora64 if mode == "r64" else [])
        request()
    times = {"none": [], "r64": []}
    for _ in range(args.reps):
        for mode in ("none", "r64"):
            dit.set_adapters(lora64 if mode == "r64" else [])
            times[mode].append(request())
    for mode, v in times.items():
        res[f"request_{mode}"] = {"median_ms": round(statistics.median(v), 2), "all_ms": [round(x, 2) for x in v]}
        print(f"metric request DiT part (8 x 30 s, 27 steps), adapter {mode}: median {statistics.median(v):.2f} ms, "
              f"runs {[round(x, 1) for x in v]}", flush=True)
    dit.close()
    print(json.dumps({"bench_lora": res}))


if __name__ == "__main__":
    main()
