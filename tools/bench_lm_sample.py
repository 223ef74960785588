#!/usr/bin/env python
"""Native LM token selection vs the reference's torch operations (same logits, same GPU, same run) -> profiles/lm_sample_bench.txt.

V = 217205 (151669 + 65536 audio-code tokens), B in (1, 8, 16); logits dense (``randn * 3``) or codes-phase (64 000 finite ids plus one
EOS id, the rest -inf); settings: the reference's default (k off, p 0.9, T 0.85), (k 50, p off), (k 200, p 0.95), all at T 0.85, and
greedy (filters off, T 0).  The torch side restates what ``LLMHandler._apply_top_k_filter``, ``_apply_top_p_filter`` and
``_sample_tokens`` run (llm_inference.py:367-399): topk + compare + indexed fill; sort, softmax, cumsum, compare, shift, scatter, indexed
fill; divide, softmax, multinomial (or argmax).  Its filters write in place, so every timed call gets a fresh copy of the logits made
outside the timed window.  The native side is ``ace355.lmsample.select_tokens(..., check=False)`` with its default ``torch.rand`` draw
of u.

Method (tools/bench_lm.py's): warm-up of both sides, then the two interleaved; device events around a batch of ``--calls`` calls, so a
sample is well out of the launch noise; microseconds per call, median [min - max] over ``--runs`` batches.  Beside it: the bytes a call
must read once (B x V x 4) over the native time, and the launches of the native chain.

Last row: one native decode step (Qwen3-0.6B shape, N = 16, length 512) plus the selection of its 8 conditional rows, both ways.

Everything is random logits; nothing here says anything about a trained LM's token stream.

Usage:  python tools/bench_lm_sample.py [--runs 15] [--calls 20] [--no-e2e] [--out profiles/lm_sample_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ace355  # noqa: E402,F401
from ace355 import lmsample  # noqa: E402

V = 151669 + 65536
SETTINGS = [("default k off p 0.9 T 0.85", None, 0.9, 0.85), ("k 50 p off T 0.85", 50, None, 0.85), ("k 200 p 0.95 T 0.85", 200, 0.95, 0.85),
            ("greedy", None, None, 0.0)]


def torch_select(logits, top_k, top_p, temperature):
    """The reference's three methods, restated; ``logits`` is modified in place as the reference modifies it."""
    if top_k is not None and top_k > 0:
        logits[logits < torch.topk(logits, top_k)[0][..., -1, None]] = float("-inf")
    if top_p is not None and 0.0 < top_p < 1.0:
        s, idx = torch.sort(logits, descending=True)
        rem = torch.cumsum(torch.softmax(s.float(), dim=-1), dim=-1) > top_p
        rem[..., 1:] = rem[..., :-1].clone()
        rem[..., 0] = 0
        logits[rem.scatter(1, idx, rem)] = float("-inf")
    if temperature > 0:
        return torch.multinomial(torch.softmax(logits.float() / temperature, dim=-1), num_samples=1).squeeze(1)
    return torch.argmax(logits, dim=-1)


def native_launches(top_k, top_p, temperature, want_mask=False):
    """The launches of ace355_lm_pick's chain (csrc/lm_sample.hip): maxima, two per level of each active filter, mask, token."""
    k_on, p_on = bool(top_k) and 0 < top_k < V, top_p is not None and 0.0 < top_p < 1.0
    masked = temperature > 0 or want_mask
    return 1 + ((6 * k_on + 6 * p_on + 1) if masked else 0) + 1


def make_logits(kind, B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 3
    if kind == "codes":
        y = torch.full((B, V), float("-inf"))
        y[:, 151669:151669 + 64000] = x[:, 151669:151669 + 64000]
        y[:, 151645] = x[:, 151645]
        x = y
    return x.to(dev)


def batch_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls   # microseconds per call


def cell(xs):
    return f"{statistics.median(xs):9.1f} [{min(xs):.1f} - {max(xs):.1f}]"


def compare(x, top_k, top_p, T, runs, calls, warmup):
    copies = [x.clone() for _ in range(calls)]

    def refill():
        for c in copies:
            c.copy_(x)
        torch.cuda.synchronize()
    f_nat = lambda i: lmsample.select_tokens(x, top_k, top_p, T, check=False)   # noqa: E731
    f_ref = lambda i: torch_select(copies[i], top_k, top_p, T)                   # noqa: E731
    for _ in range(warmup):
        batch_time(f_nat, calls)
        refill()
        batch_time(f_ref, calls)
    tn, tr = [], []
    for _ in range(runs):
        tn.append(batch_time(f_nat, calls))
        refill()
        tr.append(batch_time(f_ref, calls))
    return tn, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15, help="timed batches per side and row")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed batch")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-e2e", action="store_true", help="skip the decode-step row (it builds the 0.6B-shape LM)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_sample_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# native LM token selection vs the reference's torch operations, V = {V}, fp32 logits, {torch.cuda.get_device_name(dev)}",
             f"# {args.warmup} warm-up batches per side, then interleaved; device events around batches of {args.calls} calls, {args.runs} "
             "batches; us per call: median [min - max]",
             "# read MB = B x V x 4, what a call must read once; GB/s = that over the native median; launches = the native chain's",
             "# random logits only: nothing here is about a trained LM's token stream",
             f"{'logits':<6} {'B':>2}  {'setting':<27} {'native us':>28} {'torch us':>30} {'torch / native':>14} {'read MB':>8} {'GB/s':>7} {'launches':>8}"]
    slower = []
    with torch.inference_mode():
        for kind in ("dense", "codes"):
            for B in (1, 8, 16):
                x = make_logits(kind, B, dev, seed=B)
                for name, k, p, T in SETTINGS:
                    tn, tr = compare(x, k, p, T, args.runs, args.calls, args.warmup)
                    mn, mr = statistics.median(tn), statistics.median(tr)
                    mb = B * V * 4 / 1e6
                    lines.append(f"{kind:<6} {B:>2}  {name:<27} {cell(tn):>28} {cell(tr):>30} {mr / mn:>13.2f}x {mb:>8.2f} {mb * 1e6 / (mn * 1e-6) / 1e9:>7.1f} "
                                 f"{native_launches(k, p, T):>8}")
                    print(lines[-1], flush=True)
                    if mn > mr:
                        slower.append(f"{kind} B={B} {name}")
                del x
                torch.cuda.empty_cache()
        if args.no_e2e:
            lines.append("# decode step + selection: not measured (--no-e2e)")
        else:
            from ace355 import weightgen
            from ace355.config import LmConfig
            from ace355.lm import NativeCausalLM
            N, P = 16, 512
            cfg = LmConfig(vocab_size=V, tie_word_embeddings=True)
            w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=0, mode="test")
            nat = NativeCausalLM(cfg, dev, max_positions=P + (2 * args.warmup + 2 * args.runs) * args.calls + 8, out_dtype=torch.float32)
            nat.load_state_dict(w)
            del w
            g = torch.Generator().manual_seed(0)
            ids = torch.randint(0, V, (N, P), generator=g).to(dev)
            nxt = torch.randint(0, V, (N,), generator=g)   # (host ids: the step copies them itself)
            nat.prefill(ids)
            name, k, p, T = SETTINGS[0]

            def step_nat(i):
                lmsample.select_tokens(nat.decode(nxt)[:N // 2], k, p, T, check=False)

            def step_ref(i):
                torch_select(nat.decode(nxt)[:N // 2], k, p, T)

            def step_only(i):
                nat.decode(nxt)
            for _ in range(args.warmup):
                batch_time(step_nat, args.calls)
                batch_time(step_ref, args.calls)
            tn, tr, ts = [], [], []
            for _ in range(args.runs):
                tn.append(batch_time(step_nat, args.calls))
                tr.append(batch_time(step_ref, args.calls))
            nat.prefill(ids)
            for _ in range(args.runs):
                ts.append(batch_time(step_only, args.calls))
            mn, mr = statistics.median(tn), statistics.median(tr)
            lines.append(f"# one native decode step (Qwen3-0.6B shape, N = {N}, length {P} ..) + the selection of its {N // 2} conditional rows ({name}), us per step:")
            lines.append(f"#   step + native selection {cell(tn)}   step + torch selection {cell(tr)}   torch / native {mr / mn:.2f}x   the step alone {cell(ts)}")
            if mn > mr:
                slower.append("decode step + selection")
            nat.close()
    lines.append("# native slower than torch at: " + (", ".join(slower) if slower else "no recorded row"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
