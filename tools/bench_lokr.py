#!/usr/bin/env python
"""LoKr merge cost and per-request cost with a LoKr adapter, at full size (24 layers, hidden 2048), on one GPU, with the LoRA merge of
the same target kinds timed beside it in the same process.

Reports (readable lines plus one JSON line, also written to --out):
  * merge ms (NativeDit.set_adapters, host clock around a synchronised call; pristine copies already made) for
      - lokr_attn_default: the reference's default LoKr configuration (LoKRConfig: q / k / v / o of both attentions, factor -1 = the
        near-square split of each dimension, linear_dim 64, W1 full, W2 decomposed at rank 64 where 64 < max(out_k, in_n) / 2 and full
        otherwise - the rule of LyCORIS' published LokrModule),
      - lokr_all10: the same on all ten target kinds,
      - lokr_all10_r64: all ten kinds with a split that leaves W2 large enough to be decomposed at rank 64 (factor 8),
      - attn_r8 and all10_r64: the LoRA merges of tools/bench_lora.py;
    with the achieved GB/s of the pristine read + live write (the float4-copy ceiling of the part is about 6300 GB/s);
  * the metric request's DiT part (8 songs x 30 s, 27 steps, CFG 7 + APG) with the default LoKr adapter against no adapter, alternating.
Usage: python tools/bench_lokr.py [--reps 5] [--out profiles/lokr_merge_bench.txt]
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
COPY_GBPS = 6300


def factorization(n: int, factor: int = -1):
    """(a, b), a <= b, a b = n: the most square split, or with factor > 0 the split a = the largest divisor of n not above factor."""
    if factor > 0:
        a = min(factor, n)
        while n % a:
            a -= 1
        return min(a, n // a), max(a, n // a)
    a = int(n ** 0.5)
    while n % a:
        a -= 1
    return a, n // a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lokr_merge_bench.txt"))
    ap.add_argument("--no-request", action="store_true", help="merge timings only")
    args = ap.parse_args()
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit, generate_latents
    from ace355.lokr import KronTerm
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
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rn(*s):
        return torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)

    def lora_terms(kinds, rank):
        return [LoraTerm(n, rn(rank, shapes[n][1]), rn(shapes[n][0], rank), 1e-4)
                for li in range(cfg.num_hidden_layers) for n in (f"layers.{li}.{k}.weight" for k in kinds)]

    def lokr_terms(kinds, factor=-1, dim=64):
        out, splits = [], {}
        for li in range(cfg.num_hidden_layers):
            for k in kinds:
                n = f"layers.{li}.{k}.weight"
                (out_l, out_k), (in_m, in_n) = factorization(shapes[n][0], factor), factorization(shapes[n][1], factor)
                low = dim < max(out_k, in_n) / 2
                splits[k] = f"{out_l}x{in_m} (x) {out_k}x{in_n}{' r' + str(dim) if low else ''}"
                if low:
                    out.append(KronTerm(n, rn(out_l, in_m), None, None, None, rn(out_k, dim), rn(dim, in_n), 1e-4))
                else:
                    out.append(KronTerm(n, rn(out_l, in_m), None, None, rn(out_k, in_n), None, None, 1e-4))
        return out, splits

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
    lokr_attn, sp_attn = lokr_terms(ATTN)
    lokr_all, sp_all = lokr_terms(ALL)
    lokr_all_r64, sp_r64 = lokr_terms(ALL, factor=8)
    say("splits, default configuration: " + ", ".join(f"{k} {v}" for k, v in sp_all.items()))
    say("splits, factor 8: " + ", ".join(f"{k} {v}" for k, v in sp_r64.items()))
    for rnd in range(2):   # twice over, interleaved: the LoRA merges beside the LoKr ones
        for label, ts in (("attn_r8", lora_terms(ATTN, 8)), ("lokr_attn_default", lokr_attn), ("all10_r64", lora_terms(ALL, 64)),
                          ("lokr_all10", lokr_all), ("lokr_all10_r64", lokr_all_r64)):
            med, best = merge_ms(ts)
            weights = sum(shapes[t.name][0] * shapes[t.name][1] for t in ts)
            gbps = 4 * weights / med / 1e6
            res[f"{label}_pass{rnd}"] = {"median_ms": round(med, 3), "min_ms": round(best, 3), "weights": weights, "hbm_GBps_at_median": round(gbps, 1)}
            say(f"merge {label} (pass {rnd}): median {med:.3f} ms, min {best:.3f} ms ({weights / 1e9:.2f} G weights, read pristine + write live: "
                f"{gbps:.0f} GB/s = {100 * gbps / COPY_GBPS:.0f} % of the {COPY_GBPS} GB/s float4 copy)")
            dit.clear_adapters()

    if not args.no_request:
        gen = torch.Generator().manual_seed(0)
        B, T, L = 8, 750, 769
        enc = torch.randn(1, L, cfg.hidden_size, generator=gen).expand(B, -1, -1).contiguous().to(dev)
        ctx = torch.cat([0.5 * torch.randn(B, T, 64, generator=gen), torch.ones(B, T, 64)], -1).to(dev)
        null = weightgen.make_null_condition_emb(cfg.hidden_size, seed=4)
        kw = dict(seed=list(range(B)), infer_steps=27, diffusion_guidance_sale=7.0)

        def request():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate_latents(dit, null, enc, ctx, **kw)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)
        for mode in ("none", "lokr"):   # warm-up of both states
            dit.set_adapters(lokr_attn if mode == "lokr" else [])
            request()
        times = {"none": [], "lokr": []}
        for _ in range(args.reps):
            for mode in ("none", "lokr"):
                dit.set_adapters(lokr_attn if mode == "lokr" else [])
                times[mode].append(request())
        for mode, v in times.items():
            res[f"request_{mode}"] = {"median_ms": round(statistics.median(v), 2), "all_ms": [round(x, 2) for x in v]}
            say(f"metric request DiT part (8 x 30 s, 27 steps), adapter {mode}: median {statistics.median(v):.2f} ms, "
                f"runs {[round(x, 1) for x in v]}")
    dit.close()
    say(json.dumps({"bench_lokr": res}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
