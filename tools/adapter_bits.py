#!/usr/bin/env python
"""The bits the adapter merge leaves in the weights, as SHA-256 lines: run it on two builds and compare the outputs line for line.

Only the public Python API is used (NativeDit.set_adapters / read_weight), so the same file runs on any build that has the three
adapter families.  Weights and terms are seeded and generated on the CPU.

  * tiny configuration (hidden 256, intermediate 768, 2 layers, 2 / 1 heads): one handle walks through
      1 lora      a rank-8 LoRA on every kind of both layers, a second term (rank 3) on one target and one term at scale 0
      2 mixed     LoRA on every other target, Kronecker terms (full, decomposed, wider than a tile) on the rest, one target dropped
      3 dora      the same with DoRA on targets of both families and both axes, one multiplier 0
      4 subset    three of those targets, one of them with DoRA
      5 empty     nothing: the base is back
    and after each call prints the hash of read_weight(name, bfloat16) of every target of both layers;
  * default configuration (24 layers, hidden 2048): one call with the default LoKr split (the near-square factorisation, W2 at rank 64
    where it is large enough) on all kinds, one hash per layer over its targets in kind order.
Usage: python tools/adapter_bits.py [--out FILE] [--no-default]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "cross_attn.q_proj", "cross_attn.k_proj",
         "cross_attn.v_proj", "cross_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
SPLITS = ((16, 16, 0, 0), (16, 64, 0, 8), (8, 32, 4, 40), (2, 1, 0, 0), (1, 1, 0, 8))   # (out_l, in_m, r1, r2)


def near_square(n):
    a = int(n ** 0.5)
    while n % a:
        a -= 1
    return a, n // a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-default", action="store_true", help="the tiny configuration only")
    args = ap.parse_args()
    import ace355
    from ace355 import native, weightgen
    from ace355.dit import NativeDit
    from ace355.dora import DoraTerm
    from ace355.lokr import KronTerm
    from ace355.lora import LoraTerm
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()

    def names_of(cfg):
        return [f"layers.{li}.{k}.weight" for li in range(cfg.num_hidden_layers) for k in KINDS]

    g = torch.Generator().manual_seed(1234)

    def rn(*s):
        return torch.randn(*s, generator=g).to(torch.bfloat16)

    def lora(n, shapes, rank=8, scale=0.05):
        return LoraTerm(n, rn(rank, shapes[n][1]), rn(shapes[n][0], rank), scale)

    def kron(n, shapes, split, scale=0.05):
        out_l, in_m, r1, r2 = split
        out_k, in_n = shapes[n][0] // out_l, shapes[n][1] // in_m
        w1 = (rn(out_l, in_m), None, None) if r1 == 0 else (None, rn(out_l, r1), rn(r1, in_m))
        w2 = (rn(out_k, in_n), None, None) if r2 == 0 else (None, rn(out_k, r2), rn(r2, in_n))
        return KronTerm(n, *w1, *w2, scale)

    def dora(n, shapes, per_input, eps, m=1.0):
        return DoraTerm(n, 1.0 + 0.25 * torch.rand(shapes[n][1 if per_input else 0], generator=g), per_input, eps, m)

    # ---- tiny
    cfg = ace355.DitConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)
    shapes = cfg.weight_shapes()
    dit = NativeDit(cfg, dev)
    dit.load_state_dict(weightgen.make_dit_weights(shapes, cfg.hidden_size, seed=7, mode="test"))
    names = names_of(cfg)
    step1 = [lora(n, shapes) for n in names] + [lora(names[3], shapes, rank=3), lora(names[5], shapes, scale=0.0)]
    add = [lora(n, shapes) if i % 2 == 0 else kron(n, shapes, SPLITS[(i // 2) % len(SPLITS)]) for i, n in enumerate(names) if i != 6]
    add.append(kron(names[1], shapes, SPLITS[1]))   # (a second Kronecker term on a target that has one)
    step3 = add + [dora(t.name, shapes, i % 4 >= 2, (2.0 ** -7, 0.0)[i % 3 == 0], 0.0 if i == 9 else (1.0, 0.6)[i % 5 == 0])
                   for i, t in enumerate(add[:-1]) if i % 3 != 2]
    sub = [names[0], names[7], names[13]]
    step4 = [t for t in add if t.name in sub] + [dora(names[7], shapes, True, 2.0 ** -7)]
    for label, terms in (("1 lora", step1), ("2 mixed", add), ("3 dora", step3), ("4 subset", step4), ("5 empty", [])):
        dit.set_adapters(terms)
        for n in names:
            say(f"tiny {label} {n} {sha(dit.read_weight(n, torch.bfloat16))}")
    dit.close()

    # ---- default configuration, default LoKr split on all kinds
    if not args.no_default:
        cfg = ace355.DitConfig()
        shapes = cfg.weight_shapes()
        dit = NativeDit(cfg, dev)
        for name, shape in shapes.items():
            wt = weightgen.make_dit_weights({name: shape}, cfg.hidden_size, seed=4, mode="test")[name]
            native.check(dit._lib.ace355_dit_load_tensor(dit._h, name.encode(), native.ptr(wt.contiguous()), 0, wt.numel(), 0), name)
        native.check(dit._lib.ace355_dit_finalize(dit._h), "finalize")
        terms = []
        for n in names_of(cfg):
            (out_l, out_k), (in_m, in_n) = near_square(shapes[n][0]), near_square(shapes[n][1])
            terms.append(kron(n, shapes, (out_l, in_m, 0, 64 if 64 < max(out_k, in_n) / 2 else 0), scale=1e-2))
        dit.set_adapters(terms)
        for li in range(cfg.num_hidden_layers):
            h = hashlib.sha256()
            for k in KINDS:
                h.update(bytes.fromhex(sha(dit.read_weight(f"layers.{li}.{k}.weight", torch.bfloat16))))
            say(f"default lokr layer {li} {h.hexdigest()}")
        dit.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
