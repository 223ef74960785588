#!/usr/bin/env python
"""DoRA merge cost at full size (24 layers, hidden 2048) on one GPU, each configuration timed beside the plain merge of the same
additive terms in the same process.

Reports (readable lines plus one JSON line, also written to --out) the merge ms (NativeDit.set_adapters, host clock around a
synchronised call; pristine copies already made; one warm-up call, then --reps calls, median and min) for
  - lokr_attn_default: the reference's default LoKr configuration (q / k / v / o of both attentions, the near-square split, W2 at rank
    64 where LyCORIS decomposes it) plain, with DoRA on the output axis and with DoRA on the input axis (eps 2^-7),
  - lokr_all10: the same on all ten target kinds, plain and with DoRA (alternating axes),
  - peft_all10_r64: a rank-64 PEFT LoRA on all ten kinds, plain and with use_dora (output axis, eps 0).
A DoRA target runs twice through its merge kernel (fp64 partial sums of squares, then the rescaled write) with a small factor kernel
in between, so the expectation is at most about 3x the plain merge of the same terms.
Usage: python tools/bench_dora.py [--reps 5] [--out profiles/dora_merge_bench.txt]
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

from tools.bench_lokr import ALL, ATTN, factorization  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dora_merge_bench.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 repetitions"
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    from ace355.dora import DoraTerm
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

    def names(kinds):
        return [f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in kinds]

    def lora_terms(kinds, rank):
        return [LoraTerm(n, rn(rank, shapes[n][1]), rn(shapes[n][0], rank), 1e-4) for n in names(kinds)]

    def lokr_terms(kinds, dim=64):
        out = []
        for n in names(kinds):
            (out_l, out_k), (in_m, in_n) = factorization(shapes[n][0]), factorization(shapes[n][1])
            if dim < max(out_k, in_n) / 2:
                out.append(KronTerm(n, rn(out_l, in_m), None, None, None, rn(out_k, dim), rn(dim, in_n), 1e-4))
            else:
                out.append(KronTerm(n, rn(out_l, in_m), None, None, rn(out_k, in_n), None, None, 1e-4))
        return out

    def dora_terms(add, per_input, eps):
        """One DoRA term per target; the magnitudes are fp32 on the device already (what the seam holds)."""
        return [DoraTerm(t.name, 1 + 0.25 * torch.randn(shapes[t.name][1 if per_input(i) else 0], device=dev, generator=g),
                         per_input(i), eps, 1.0) for i, t in enumerate(add)]

    def merge_ms(ts):
        dit.set_adapters(ts)   # (warm-up; first touch: pristine copies)
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dit.set_adapters(ts)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times), min(times)

    lokr_attn, lokr_all, peft_all = lokr_terms(ATTN), lokr_terms(ALL), lora_terms(ALL, 64)
    out_axis, in_axis, alt = (lambda i: False), (lambda i: True), (lambda i: i % 2 == 1)
    configs = (
        ("lokr_attn_default", lokr_attn, (("dora_out", dora_terms(lokr_attn, out_axis, 2.0 ** -7)),
                                          ("dora_in", dora_terms(lokr_attn, in_axis, 2.0 ** -7)))),
        ("lokr_all10", lokr_all, (("dora_alternating_axes", dora_terms(lokr_all, alt, 2.0 ** -7)),)),
        ("peft_all10_r64", peft_all, (("use_dora", dora_terms(peft_all, out_axis, 0.0)),)),
    )
    res = {}
    for rnd in range(2):   # twice over, interleaved: every DoRA merge beside the plain merge of the same additive terms
        for label, add, variants in configs:
            weights = sum(shapes[t.name][0] * shapes[t.name][1] for t in add)
            med0, best0 = merge_ms(add)
            res[f"{label}_plain_pass{rnd}"] = {"median_ms": round(med0, 3), "min_ms": round(best0, 3), "weights": weights}
            say(f"merge {label} plain (pass {rnd}): median {med0:.3f} ms, min {best0:.3f} ms ({weights / 1e9:.2f} G weights)")
            for vlabel, dora in variants:
                med, best = merge_ms(add + dora)
                res[f"{label}_{vlabel}_pass{rnd}"] = {"median_ms": round(med, 3), "min_ms": round(best, 3), "x_plain": round(med / med0, 2)}
                say(f"merge {label} + {vlabel} (pass {rnd}): median {med:.3f} ms, min {best:.3f} ms = {med / med0:.2f} x the plain merge")
            dit.clear_adapters()
    dit.close()
    say(json.dumps({"bench_dora": res}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
