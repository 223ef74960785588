#!/usr/bin/env python
"""B songs in one batched CFG loop vs the same B songs through B sequential native loops (same LM, same GPU, same run)
-> profiles/lm_batch_bench.txt.

Shape: Qwen3-0.6B with V = 217205 (151669 + 65536 audio-code tokens), random weights, prompt 512, the reference's default settings
(cfg_scale 2, top-p 0.9, T 0.85, repetition penalty 1, no codes temperature), a codes-phase request of 150 and of 1200 codes,
B = 2 / 4 / 8 songs with one prompt and B seeds - the reference's only batch caller (llm_inference.py:1314-1373).

* batched: ``ace355.lmlogits.generate_codes_batch`` - one prefill of the [2, P] pair, ``fan_out``, one loop over 2B sequences.
* sequential: what ``_run_pt`` does on the native loop, the parent's behaviour: per song ``torch.manual_seed(seed)``, a processor
  reset, and ``NativeLmMixin._generate_with_cfg_custom`` (``use_native_lm_loop``) on the pair.

Both sides run whole requests, prefill included, and are timed with the host clock between two device synchronisations; one warm-up
request per side, then interleaved.  Song i of the batched call equals sequential song i token for token, which the tool asserts.

Second table: the pair's prefill plus ``fan_out`` against the [2B, P] prefill it replaces (host clock between synchronisations; the
fan-out alone also by device events).

Random weights only; nothing here says anything about a trained LM's token stream.

Usage:  python tools/bench_lm_batch.py [--runs 3] [--long 1200] [--out profiles/lm_batch_bench.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ace355  # noqa: E402,F401
import _lm_loop_ref as R  # noqa: E402  (the processor's codes-phase branches, restated)
from ace355 import lmlogits  # noqa: E402
from ace355.backend import NativeLmMixin  # noqa: E402

V = 151669 + 65536
EOS, PAD, CODE0, CODES = 151645, 151643, 151669, 64000
P = 512
CFG, TOP_P, TEMP = 2.0, 0.9, 0.85


class _Tok:
    eos_token_id = EOS


class _Base:
    def _build_logits_processor(self, repetition_penalty):
        return [] if repetition_penalty == 1.0 else [lambda ids, s: R.repetition_penalty(ids, s, repetition_penalty)]


class Handler(NativeLmMixin, _Base):
    pass


def reset(proc, target):
    """``MetadataConstrainedLogitsProcessor.reset`` + ``set_target_duration`` as far as the codes phase goes."""
    proc.state, proc.codes_count, proc.target_codes = R.FSMState.THINK_TAG, 0, target
    return proc


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cell(xs, w=9):
    return f"{statistics.median(xs):{w}.1f} [{min(xs):.1f} - {max(xs):.1f}]"


def pair_prompt(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (2, P), generator=g).to(dev)
    ids[0, -2:] = torch.tensor(R.THINK_END, device=dev)
    return ids, torch.ones_like(ids)


def loop_rows(lm, dev, proc, B, codes, runs, lines, slower):
    ids, am = pair_prompt(dev, B)
    h = Handler()
    h.llm, h.device, h.use_native_lm_loop, h.llm_tokenizer = lm, dev, True, _Tok()
    seeds = [1000 + 17 * i for i in range(B)]
    max_new = codes + 10

    def batched():
        return lmlogits.generate_codes_batch(h, lm, ids, am, seeds, max_new, TEMP, CFG, None, TOP_P, 1.0, PAD, reset(proc, codes))

    def sequential():
        rows = []
        for s in seeds:
            torch.manual_seed(s)
            torch.cuda.manual_seed_all(s)
            rows.append(h._generate_with_cfg_custom(ids, am, max_new, TEMP, CFG, None, TOP_P, 1.0, PAD, None, reset(proc, codes))[0])
        return torch.stack(rows)
    a, b = batched(), sequential()       # warm-up of both, and the agreement
    assert torch.equal(a, b) and a.shape == (B, P + codes + 1), (a.shape, b.shape)
    tb, ts = [], []
    for _ in range(runs):
        tb.append(timed(batched)[0])
        ts.append(timed(sequential)[0])
    mb, ms = statistics.median(tb), statistics.median(ts)
    mark = "" if mb <= ms else "   **batched slower**"
    lines.append(f"{B:>2} {2 * B:>3} {codes:>6}  {cell(tb):>32} {cell(ts):>32} {ms / mb:>8.2f}x {mb / (codes + 1):>10.3f} "
                 f"{mb / (codes + 1) / B:>10.3f}{mark}")
    print(lines[-1], flush=True)
    if mb > ms:
        slower.append(f"loop B={B} codes={codes}")


def prefill_rows(lm, dev, B, runs, lines, slower):
    ids, am = pair_prompt(dev, B)
    wide_ids = torch.cat([ids[:1].expand(B, P), ids[1:].expand(B, P)]).contiguous()
    wide_am = torch.ones_like(wide_ids)
    src = [0] * B + [1] * B

    def fanned():
        lm.prefill(ids, am)
        lm.fan_out(src)

    def wide():
        lm.prefill(wide_ids, wide_am)
    fanned(), wide()
    tf, tw, to = [], [], []
    for _ in range(runs):
        tf.append(timed(fanned)[0])
        tw.append(timed(wide)[0])
        lm.prefill(ids, am)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lm.fan_out(src)
        e1.record()
        e1.synchronize()
        to.append(e0.elapsed_time(e1))
    mf, mw = statistics.median(tf), statistics.median(tw)
    mark = "" if mf <= mw else "   **fan-out slower**"
    lines.append(f"{B:>2} {2 * B:>3}  {cell(tf, 8):>28} {cell(to, 8):>28} {cell(tw, 8):>28} {mw / mf:>8.2f}x{mark}")
    print(lines[-1], flush=True)
    if mf > mw:
        slower.append(f"prefill B={B}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3, help="timed requests per side and row")
    ap.add_argument("--codes", type=int, default=150)
    ap.add_argument("--long", type=int, default=1200, help="codes of the long runs (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_batch_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from ace355 import weightgen
    from ace355.config import LmConfig
    from ace355.lm import NativeCausalLM
    cfg = LmConfig(vocab_size=V, tie_word_embeddings=True)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=0, mode="test")
    lm = NativeCausalLM(cfg, dev, max_positions=P + max(args.codes, args.long) + 16, out_dtype=torch.float32)
    lm.load_state_dict(w)
    del w
    proc = R.CodesProcessor(V, range(CODE0, CODE0 + CODES), EOS, target_codes=args.codes)
    lines = [f"# B songs in one batched CFG loop vs B sequential native loops, Qwen3-0.6B shape, V = {V}, prompt {P}, {torch.cuda.get_device_name(dev)}",
             f"# cfg_scale {CFG}, top-p {TOP_P}, T {TEMP}, penalty 1; one prompt, B seeds; whole request incl. prefill, host clock between",
             f"# device synchronisations, one warm-up request per side, then {args.runs} interleaved ({max(1, args.runs - 1)} for the long runs); ms per request: median [min - max]",
             "# sequential = per song: torch.manual_seed, processor reset, the native loop on the [2, P] pair (the parent's behaviour);",
             "# batched song i = sequential song i token for token (asserted)",
             "# random weights only: nothing here is about a trained LM's token stream",
             f"{'B':>2} {'N':>3} {'codes':>6}  {'batched ms/request':>32} {'sequential ms/request':>32} {'seq / bat':>9} {'ms/step':>10} {'ms/song-tok':>10}"]
    slower = []
    for B in (2, 4, 8):
        loop_rows(lm, dev, proc, B, args.codes, args.runs, lines, slower)
    if args.long:
        for B in (2, 4, 8):
            loop_rows(lm, dev, proc, B, args.long, max(1, args.runs - 1), lines, slower)
    lines += ["#", f"# prefill of the [2, {P}] pair + fan_out vs the [2B, {P}] prefill it replaces; host clock between synchronisations, ms: median [min - max];",
              "# fan_out alone by device events",
              f"{'B':>2} {'N':>3}  {'pair prefill + fan_out':>28} {'fan_out alone':>28} {'[2B, P] prefill':>28} {'wide / fan':>9}"]
    for B in (2, 4, 8):
        prefill_rows(lm, dev, B, max(args.runs, 5), lines, slower)
    lm.close()
    lines.append("# batched slower at: " + (", ".join(slower) if slower else "no recorded row"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
