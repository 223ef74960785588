#!/usr/bin/env python
"""The workload behind the decode-attention figures of profiles/lm_gqa4_bench.txt: the same decode steps on a 4 : 1 and on a 2 : 1 stack.

Two small stacks with the SAME kv heads (8), layers (2) and cache (N = 16 sequences, length 2048 -> 2048 + steps), one with 32 q heads
(``allow_gqa4=True``) and one with 16, each prefilled once and then stepped.  The K / V bytes a decode-attention launch reads are equal
on the two, so the ratio of ``decode_attn_kernel<4>`` to ``decode_attn_kernel<2>`` time says whether the kernel is still bound by them.
Run it under a kernel trace, which names the two instantiations apart:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lm_gqa4_trace.py

Without a profiler it prints the wall time per step of each stack (GEMMs included: not the figure above).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ace355  # noqa: E402,F401
from ace355 import weightgen  # noqa: E402
from ace355.config import LmConfig  # noqa: E402
from ace355.lm import NativeCausalLM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--length", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for heads in (32, 16):
        cfg = LmConfig(hidden_size=768, intermediate_size=1216, num_hidden_layers=2, num_attention_heads=heads, num_key_value_heads=8,
                       vocab_size=2051, tie_word_embeddings=True)
        lm = NativeCausalLM(cfg, dev, max_positions=args.length + args.steps + 1, max_seqs=args.seqs, allow_gqa4=True)
        lm.load_state_dict(weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=heads, mode="test"))
        ids = torch.randint(0, cfg.vocab_size, (args.seqs, args.length), generator=g)
        lm.prefill(ids)
        nxt = torch.randint(0, cfg.vocab_size, (args.seqs,), generator=g).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lm.decode_tokens(nxt)
        torch.cuda.synchronize()
        print(f"{heads} / 8 heads, N = {args.seqs}, length {args.length}: {(time.perf_counter() - t0) / args.steps * 1e3:.3f} ms per decode step "
              f"({cfg.num_hidden_layers} layers)", flush=True)
        lm.close()


if __name__ == "__main__":
    main()
