#!/usr/bin/env python
"""Teacher-forced LM scoring: native ``NativeCausalLM.score`` vs the reference's path, same weights, same GPU -> profiles/lm_score_bench.txt.

The Qwen3-0.6B shape (28 layers, hidden 1024, tied head, vocabulary 151669 + 65536 = 217205) with weightgen "test" weights.  One row per
(prompt, target): prompts of 256 and 1300 tokens (the understanding prompt around 150 and 1200 audio codes), targets of 16, 64 and 512
tokens (a metadata field, a caption, lyrics).  Per row:

* native: one ``score`` call, unpadded N = 1 - upload, embedding, the stack over all P positions, the three head launches on the T target
  rows - and the read-back of T log-probs and ranks;
* head alone: ``ace355_lm_score_rows`` on T random rows against a [V, D] head, device events around the three launches, beside its model:
  W read once at 6.3 TB/s plus 2 T V D FLOPs at the dense bf16 peak (2.5 PFLOP/s) - whichever is larger bounds it;
* reference, restated here from acestep/core/scoring/lm_score.py: transformers' bf16 forward over all P positions (all P x V logits), the
  [T, V] slice to the host, then ``log_softmax`` + gather (the PMI path) or ``topk(10)`` (the recall path) there.

Each side is warmed up, then the sides run interleaved; host clock around work that ends in a synchronise or a host copy; ms per call,
median [min - max].  No speed-up is promised: the last line names the rows at which native is slower.

Usage:  python tools/bench_lm_score.py [--runs 5] [--out profiles/lm_score_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ace355  # noqa: E402,F401
from ace355 import lmscore, weightgen  # noqa: E402
from ace355.config import LmConfig  # noqa: E402
from ace355.lm import NativeCausalLM  # noqa: E402
from bench_lm import hf_model  # noqa: E402

PROMPTS, TARGETS = (256, 1300), (16, 64, 512)
HBM_BYTES_PER_S, BF16_FLOPS = 6.3e12, 2.5e15


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cell(xs):
    return f"{statistics.median(xs):9.3f} [{min(xs):.3f} - {max(xs):.3f}]" if xs else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_score_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_score needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    cfg = LmConfig(vocab_size=151669 + 65536, tie_word_embeddings=True)
    V, D = cfg.vocab_size, cfg.hidden_size
    w = weightgen.make_dit_weights(cfg.weight_shapes(), D, seed=0, mode="test")
    nat = NativeCausalLM(cfg, dev, max_positions=max(PROMPTS) + max(TARGETS) + 8, max_seqs=1)
    nat.load_state_dict(w)
    ref, note = hf_model(cfg, w, dev)
    head = w["model.embed_tokens.weight"].to(dev, torch.bfloat16).contiguous()
    del w
    g = torch.Generator().manual_seed(0)
    lines = [f"# LM scoring, Qwen3-0.6B shape ({cfg.num_hidden_layers} layers, hidden {D}, vocabulary {V}, tied head), "
             f"{torch.cuda.get_device_name(dev)}", f"# {note}",
             f"# {args.warmup} warm-up calls per side, then {args.runs} interleaved runs; ms per call: median [min - max]",
             f"# head model: W ({2 * V * D / 1e6:.0f} MB) once at {HBM_BYTES_PER_S / 1e12:.1f} TB/s, or 2 T V D FLOPs at "
             f"{BF16_FLOPS / 1e15:.1f} PFLOP/s, whichever is larger",
             f"{'prompt + target':<16} {'native score':>30} {'head alone':>28} {'model':>7} {'ref log_softmax path':>30} {'ref topk path':>30} "
             f"{'ref / native':>13}"]
    slower = []
    with torch.inference_mode():
        for P0 in PROMPTS:
            for T in TARGETS:
                P = P0 + T
                ids = torch.randint(0, V, (1, P), generator=g)
                ids_dev, mask_dev = ids.to(dev), torch.ones(1, P, dtype=torch.long, device=dev)
                tids = ids[0, P0:]
                x = torch.randn(T, D, generator=g).to(dev, torch.bfloat16)
                t32 = tids.to(dev, torch.int32)

                def f_nat():
                    lp, rank = nat.score(ids, None, start=P0)
                    return lp.cpu(), rank.cpu()

                def f_head():
                    return lmscore.score_rows(x, head, t32)

                def f_ref(topk):
                    logits = ref(input_ids=ids_dev, attention_mask=mask_dev).logits
                    tl = logits[0, P0 - 1:-1, :].cpu()
                    if topk:
                        return torch.topk(tl, k=10, dim=-1)
                    return torch.nn.functional.log_softmax(tl, dim=-1)[torch.arange(T), tids].mean().item()

                sides = [("nat", f_nat, wall), ("head", f_head, events)]
                if ref is not None:
                    sides += [("lsm", lambda: f_ref(False), wall), ("topk", lambda: f_ref(True), wall)]
                ts = {k: [] for k, _f, _t in sides}
                for i in range(args.warmup + args.runs):
                    for k, f, timer in sides:
                        ms = timer(f)
                        if i >= args.warmup:
                            ts[k].append(ms)
                model_ms = max(2 * V * D / HBM_BYTES_PER_S, 2.0 * T * V * D / BF16_FLOPS) * 1e3
                ratio = "-"
                if ref is not None:
                    r = min(statistics.median(ts["lsm"]), statistics.median(ts["topk"])) / statistics.median(ts["nat"])
                    ratio = f"{r:.2f}x"
                    if r < 1.0:
                        slower.append(f"{P0} + {T}")
                lines.append(f"{f'{P0} + {T}':<16} {cell(ts['nat']):>30} {cell(ts['head']):>28} {model_ms:7.3f} {cell(ts.get('lsm')):>30} "
                             f"{cell(ts.get('topk')):>30} {ratio:>13}")
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    lines.append("# native slower than the reference path at: " + (", ".join(slower) if slower else "no recorded row"))
    nat.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
