#!/usr/bin/env python
"""The device-resident CFG loop vs what the loop was before it (same LM, same GPU, same run) -> profiles/lm_loop_bench.txt.

Shape: Qwen3-0.6B with V = 217205 (151669 + 65536 audio-code tokens), random weights, prompt 512, B = 1 and 8 (N = 2 / 16 sequences),
the reference's default settings (cfg_scale 2, top-p 0.9, T 0.85, repetition penalty 1, no codes temperature), a codes-phase request
with a target duration: 150 codes, and one 1200-code run at B = 8.

* native: ``NativeLmMixin._generate_with_cfg_custom`` with ``use_native_lm_loop`` (ace355.lmlogits.generate_with_cfg).
* before: a RESTATEMENT of what the loop was, not the reference's code path itself (the reference is not importable where this runs):
  the reference's loop (llm_inference.py:2414-2533) written out below line by line, on the native forward through
  ``NativeCausalLM.__call__`` (what ``_forward_pass`` reaches through the swap) with the native selection as the seam calls it under
  ``ACE355_LM_SAMPLER=1`` (``select_tokens`` with its check): the torch CFG combine, the processor's torch operations (restated in
  tests/_lm_loop_ref.py), ``.item()`` per row, two ``torch.any``, two ``torch.cat`` per token.  Not restated: tqdm, the swap module's
  dispatch, the seam's bookkeeping of deferred filters - all host work the real path adds on top.

Both loops run the whole request, prefill included, and are timed with the host clock between two device synchronisations (the host
is what the change is about); ms per token = that time over the steps.  Warm-up of both sides, then interleaved.  The two draws agree
token for token (same seed, same selection), which the tool asserts.

Second table: ``shape_logits`` against the torch operations it replaces, us per call at B = 1 / 8 / 16 (device events around batches
of calls), beside the stage's byte floor: reads 2 B V x 4 + the mask, writes B V x 4, at 6.3 TB/s.

Random weights and random logits only; nothing here says anything about a trained LM's token stream.

Usage:  python tools/bench_lm_loop.py [--runs 3] [--long 1200] [--out profiles/lm_loop_bench.txt]
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
import _lm_loop_ref as R  # noqa: E402  (the processor's codes-phase branches and the penalty, restated)
from ace355 import lmlogits, lmsample  # noqa: E402
from ace355.backend import NativeLmMixin  # noqa: E402

V = 151669 + 65536
EOS, PAD, CODE0, CODES = 151645, 151643, 151669, 64000
P = 512
CFG, TOP_P, TEMP = 2.0, 0.9, 0.85
HBM = 6.3e12


class _Tok:
    eos_token_id = EOS


class _Base:
    def _build_logits_processor(self, repetition_penalty):
        return [] if repetition_penalty == 1.0 else [lambda ids, s: R.repetition_penalty(ids, s, repetition_penalty)]


class Handler(NativeLmMixin, _Base):
    pass


def processor(target):
    return R.CodesProcessor(V, range(CODE0, CODE0 + CODES), EOS, target_codes=target)


def before_loop(lm, ids, am, max_new, proc, pen):
    """llm_inference.py:2438-2533 with ``self.llm`` = the native LM and the three selection methods = ``select_tokens``."""
    B = ids.shape[0] // 2
    generated_ids, attention_mask = ids.clone(), am.clone()
    kv = None
    with torch.inference_mode():
        for _step in range(max_new):
            if kv is None:
                out = lm(input_ids=generated_ids, attention_mask=attention_mask, use_cache=True)
            else:
                out = lm(input_ids=generated_ids[:, -1:], past_key_values=kv, attention_mask=attention_mask, use_cache=True)
            logits = out.logits[:, -1, :]
            cond, uncond = logits[:B], logits[B:]
            x = uncond.float() + CFG * (cond.float() - uncond.float())
            cur = generated_ids[:B]
            x = proc(cur, x)
            if pen != 1.0:
                x = R.repetition_penalty(cur, x, pen)
            tokens = lmsample.select_tokens(x, None, TOP_P, TEMP)   # check=True: NativeLmMixin._sample_tokens' call, one more read
            for b in range(B):
                proc.update_state(tokens[b].item())
            stop = bool(torch.any(tokens == EOS)) or bool(torch.any(tokens == PAD))
            generated_ids = torch.cat([generated_ids, tokens.unsqueeze(1).repeat(2, 1)], dim=1)
            attention_mask = torch.cat([attention_mask, torch.ones((2 * B, 1), device=ids.device, dtype=attention_mask.dtype)], dim=1)
            kv = out.past_key_values
            if stop:
                break
    return generated_ids


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cell(xs, w=8):
    return f"{statistics.median(xs):{w}.3f} [{min(xs):.3f} - {max(xs):.3f}]"


def loop_rows(lm, dev, B, codes, runs, lines, slower):
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(0, 1000, (2 * B, P), generator=g).to(dev)
    ids[:B, -2:] = torch.tensor(R.THINK_END, device=dev)
    am = torch.ones_like(ids)
    h = Handler()
    h.llm, h.device, h.use_native_lm_loop, h.llm_tokenizer = lm, dev, True, _Tok()
    target, max_new = codes * B, codes + 8     # the count advances by B per step (one update_state per row)

    def native():
        torch.manual_seed(1)
        return h._generate_with_cfg_custom(ids, am, max_new, TEMP, CFG, None, TOP_P, 1.0, PAD, None, processor(target))

    def before():
        torch.manual_seed(1)
        return before_loop(lm, ids, am, max_new, processor(target), 1.0)
    a, b = native(), before()       # warm-up of both, and the agreement
    assert torch.equal(a, b) and a.shape[1] == P + codes + 1, (a.shape, b.shape)
    stats = dict(h._lm_loop_stats)
    tn, tb = [], []
    for _ in range(runs):
        tn.append(timed(native)[0] / (codes + 1))
        tb.append(timed(before)[0] / (codes + 1))
    mn, mb = statistics.median(tn), statistics.median(tb)
    mark = "" if mn <= mb else "   **native slower**"
    lines.append(f"{B:>2} {2 * B:>3} {codes:>6}  {cell(tn):>30} {cell(tb):>30} {mb / mn:>8.2f}x   {stats['token_reads']:>5} {stats['sync_free_steps']:>9}{mark}")
    print(lines[-1], flush=True)
    if mn > mb:
        slower.append(f"loop B={B} codes={codes}")


def torch_stage(cond, uncond, mask, eos, T, pen, cur):
    x = uncond.float() + CFG * (cond.float() - uncond.float())
    x = x + mask
    x[:, eos] = float("-inf")
    if T is not None:
        x = x / T
    if pen != 1.0:
        x = R.repetition_penalty(cur, x, pen)
    return x


def batch_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def stage_rows(dev, runs, calls, lines, slower):
    mask = torch.full((V,), float("-inf"), device=dev)
    mask[CODE0:CODE0 + CODES] = 0
    mask[EOS] = 0
    for B in (1, 8, 16):
        logits = torch.randn(2 * B, V, device=dev) * 3
        cur = torch.randint(0, V, (B, P + 150), device=dev)
        seen = lmlogits.SeenTokens(B, V, dev).mark(cur)
        out = torch.empty(B, V, device=dev)
        for name, T, pen in (("default: CFG, mask, EOS blocked", None, 1.0), ("+ codes temperature 0.85, penalty 1.1", 0.85, 1.1)):
            f_nat = lambda: lmlogits.shape_logits(logits[:B], logits[B:], CFG, mask, EOS, 1, T, pen, seen, out=out)   # noqa: E731
            f_ref = lambda: torch_stage(logits[:B], logits[B:], mask[None, :], EOS, T, pen, cur)                        # noqa: E731
            for _ in range(2):
                batch_time(f_nat, calls), batch_time(f_ref, calls)
            tn, tr = [], []
            for _ in range(runs):
                tn.append(batch_time(f_nat, calls))
                tr.append(batch_time(f_ref, calls))
            mn, mr = statistics.median(tn), statistics.median(tr)
            floor = (3 * B * V * 4 + V * 4) / HBM * 1e6
            mark = "" if mn <= mr else "   **native slower**"
            lines.append(f"{B:>2}  {name:<40} {cell(tn, 7):>26} {cell(tr, 7):>28} {mr / mn:>8.2f}x {floor:>9.2f} {mn / floor:>8.1f}x{mark}")
            print(lines[-1], flush=True)
            if mn > mr:
                slower.append(f"stage B={B} {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3, help="timed requests per side and row")
    ap.add_argument("--codes", type=int, default=150)
    ap.add_argument("--long", type=int, default=1200, help="codes of the long run at B = 8 (0: skip)")
    ap.add_argument("--stage-runs", type=int, default=15)
    ap.add_argument("--stage-calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_loop_bench.txt"))
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
    lines = [f"# the device-resident CFG loop vs the loop before it, Qwen3-0.6B shape, V = {V}, prompt {P}, {torch.cuda.get_device_name(dev)}",
             f"# cfg_scale {CFG}, top-p {TOP_P}, T {TEMP}, penalty 1; a codes-phase request with a target; whole request incl. prefill, host clock",
             f"# between device synchronisations, one warm-up request per side, then {args.runs} interleaved; ms per token: median [min - max]",
             "# before = the reference's loop RESTATED in the tool, on the native forward (NativeCausalLM.__call__) with the native selection",
             "# as the seam calls it (select_tokens with its check); same tokens as the native loop (asserted)",
             "# random weights only: nothing here is about a trained LM's token stream",
             f"{'B':>2} {'N':>3} {'codes':>6}  {'native ms/token':>30} {'before ms/token':>30} {'before / native':>9}   {'reads':>5} {'sync-free':>9}"]
    slower = []
    for B in (1, 8):
        loop_rows(lm, dev, B, args.codes, args.runs, lines, slower)
    if args.long:
        loop_rows(lm, dev, 8, args.long, max(1, args.runs - 1), lines, slower)
    lm.close()
    torch.cuda.empty_cache()
    lines += ["#", f"# shape_logits vs the torch operations it replaces, V = {V}; device events around batches of {args.stage_calls} calls, "
              f"{args.stage_runs} batches; us per call: median [min - max]",
              "# floor us = (2 B V x 4 + V x 4 read, B V x 4 written) at 6.3 TB/s",
              f"{'B':>2}  {'setting':<40} {'native us':>26} {'torch us':>28} {'torch / native':>9} {'floor us':>9} {'native / floor':>9}"]
    with torch.inference_mode():
        stage_rows(dev, args.stage_runs, args.stage_calls, lines, slower)
    lines.append("# native slower at: " + (", ".join(slower) if slower else "no recorded row"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
