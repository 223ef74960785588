#!/usr/bin/env python
"""The native non-CFG loop of the 5 Hz LM vs what that loop was before it, B songs in one batched non-CFG loop vs B sequential native
loops, and the stage alone at both dtypes (same LM, same GPU, same run) -> profiles/lm_nocfg_bench.txt.

Shape: Qwen3-0.6B with V = 217205 (151669 + 65536 audio-code tokens), random weights, ``out_dtype`` bf16, prompt 512, the reference's
default settings without CFG (top-p 0.9, T 0.85, repetition penalty 1, no codes temperature).

(a) B = 1: a free phase of 300 tokens (``generation_phase="understand"``, state ``COMPLETED`` with the ``audio_code_mask``: what
    understand_audio_from_codes / create_sample_from_query / format_sample_from_input run after their metadata) and codes phases of
    150 and 1200 codes.
    * native: ``NativeLmMixin._generate_with_constrained_decoding`` with ``use_native_lm_nocfg`` (ace355.lmlogits.generate_constrained).
    * before: the loop before it on the same host, restated here: the reference's ``_generate_with_constrained_decoding``
      (llm_inference.py:2321-2412) over the native forward (``lm(...)``, logits in bf16) and the native selection
      (``select_tokens``), with the processor's and the penalty's torch operations in bf16 in between, ``.item()`` per row, two
      ``torch.any``, two ``torch.cat`` per token.  Not restated: tqdm.
    Both draw from the same torch seed; whether the two sides produced equal tokens is reported, not asserted: torch on the GPU may
    divide by a host scalar through its reciprocal (include/ace355.h above ace355_lm_shape_as), which the default settings here never do.
(b) 150 / 1200 codes for B = 2 / 4 / 8 / 16 songs with one prompt and B seeds: ``generate_codes_batch_nocfg`` vs B sequential native
    non-CFG loops (per song ``torch.manual_seed(seed)`` and a processor reset).  Song i of the batched call equals sequential song i
    token for token, which the tool asserts.
(c) The stage alone per call (device events over batches of calls), ``shape_logits`` at both dtypes against the torch operations it
    replaces at that dtype.

Whole requests, prefill included, host clock between two device synchronisations; one warm-up request per side, then interleaved.
Random weights only; nothing here says anything about a trained LM's token stream.

Usage:  python tools/bench_lm_nocfg.py [--runs 3] [--long 1200] [--out profiles/lm_nocfg_bench.txt]
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
import _lm_loop_ref as R  # noqa: E402  (the processor's branches and the penalty, restated)
from ace355 import lmlogits, lmsample  # noqa: E402
from ace355.backend import NativeLmMixin  # noqa: E402

V = 151669 + 65536
EOS, PAD, CODE0, CODES = 151645, 151643, 151669, 64000
P = 512
TOP_P, TEMP = 0.9, 0.85


class _Tok:
    eos_token_id = EOS


class _Base:
    def _build_logits_processor(self, repetition_penalty):
        return [] if repetition_penalty == 1.0 else [lambda ids, s: R.repetition_penalty(ids, s, repetition_penalty)]

    def _generate_with_constrained_decoding(self, *a, **k):
        raise AssertionError("the request did not fit the native loop")


class Handler(NativeLmMixin, _Base):
    pass


def handler(lm, dev):
    h = Handler()
    h.llm, h.device, h.use_native_lm_nocfg, h.llm_tokenizer = lm, dev, True, _Tok()
    return h


def codes_processor(target):
    return R.CodesProcessor(V, range(CODE0, CODE0 + CODES), EOS, target_codes=target)


def free_processor():
    """The "understand" phase after its metadata: ``COMPLETED``, audio codes blocked, EOS open."""
    p = R.CodesProcessor(V, range(CODE0, CODE0 + CODES), EOS, generation_phase="understand")
    m = torch.zeros(1, V)
    m[0, CODE0:CODE0 + CODES] = float("-inf")
    p.audio_code_mask, p.state = m, R.FSMState.COMPLETED
    return p


def before_loop(lm, ids, am, max_new, proc, pen):
    """llm_inference.py:2342-2412 with ``self.llm`` = the native LM and the three selection methods = ``select_tokens``."""
    B = ids.shape[0]
    generated_ids, attention_mask = ids.clone(), am.clone()
    kv = None
    with torch.inference_mode():
        for _step in range(max_new):
            if kv is None:
                out = lm(input_ids=generated_ids, attention_mask=attention_mask, use_cache=True)
            else:
                out = lm(input_ids=generated_ids[:, -1:], past_key_values=kv, attention_mask=attention_mask, use_cache=True)
            x = out.logits[:, -1, :]                                # the model's dtype: no upcast
            x = proc(generated_ids, x)
            if pen != 1.0:
                x = R.repetition_penalty(generated_ids, x, pen)
            tokens = lmsample.select_tokens(x.float(), None, TOP_P, TEMP)   # check=True: NativeLmMixin._sample_tokens' call, one more read
            for b in range(B):
                proc.update_state(tokens[b].item())
            stop = bool(torch.any(tokens == EOS)) or bool(torch.any(tokens == PAD))
            generated_ids = torch.cat([generated_ids, tokens.unsqueeze(1)], dim=1)
            attention_mask = torch.cat([attention_mask, torch.ones((B, 1), device=ids.device, dtype=attention_mask.dtype)], dim=1)
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


def cell(xs, w=9, d=1):
    return f"{statistics.median(xs):{w}.{d}f} [{min(xs):.{d}f} - {max(xs):.{d}f}]"


def prompt(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (1, P), generator=g).to(dev)
    ids[0, -2:] = torch.tensor(R.THINK_END, device=dev)
    return ids, torch.ones_like(ids)


def single_rows(lm, dev, name, make_proc, tokens, runs, lines, slower):
    ids, am = prompt(dev, 1)
    h = handler(lm, dev)
    max_new = tokens if name == "free" else tokens + 8

    def native():
        torch.manual_seed(1)
        return h._generate_with_constrained_decoding(ids, am, max_new, TEMP, None, TOP_P, 1.0, PAD, None, make_proc())

    def before():
        torch.manual_seed(1)
        return before_loop(lm, ids, am, max_new, make_proc(), 1.0)
    a, b = native(), before()       # warm-up of both
    same = a.shape == b.shape and bool(torch.equal(a, b))
    steps = a.shape[1] - P
    stats = dict(h._lm_loop_stats)
    tn, tb = [], []
    for _ in range(runs):
        tn.append(timed(native)[0] / steps)
        tb.append(timed(before)[0] / (b.shape[1] - P))
    mn, mb = statistics.median(tn), statistics.median(tb)
    mark = "" if mn <= mb else "   **native slower**"
    lines.append(f"{name:<6} {steps:>6}  {cell(tn, 8, 3):>30} {cell(tb, 8, 3):>30} {mb / mn:>8.2f}x   {stats['token_reads']:>5} "
                 f"{stats['sync_free_steps']:>9}   {'yes' if same else 'NO'}{mark}")
    print(lines[-1], flush=True)
    if mn > mb:
        slower.append(f"loop {name} {tokens}")


def batch_rows(lm, dev, B, codes, runs, lines, slower):
    ids, am = prompt(dev, B)
    h = handler(lm, dev)
    seeds = [1000 + 17 * i for i in range(B)]
    max_new = codes + 10

    def batched():
        return lmlogits.generate_codes_batch_nocfg(h, lm, ids, am, seeds, max_new, TEMP, None, TOP_P, 1.0, PAD, codes_processor(codes))

    def sequential():
        rows = []
        for s in seeds:
            torch.manual_seed(s)
            torch.cuda.manual_seed_all(s)
            rows.append(h._generate_with_constrained_decoding(ids, am, max_new, TEMP, None, TOP_P, 1.0, PAD, None, codes_processor(codes))[0])
        return torch.stack(rows)
    a, b = batched(), sequential()       # warm-up of both, and the agreement
    assert torch.equal(a, b) and a.shape == (B, P + codes + 1), (a.shape, b.shape)
    tb, ts = [], []
    for _ in range(runs):
        tb.append(timed(batched)[0])
        ts.append(timed(sequential)[0])
    mb, ms = statistics.median(tb), statistics.median(ts)
    mark = "" if mb <= ms else "   **batched slower**"
    lines.append(f"{B:>2} {codes:>6}  {cell(tb):>32} {cell(ts):>32} {ms / mb:>8.2f}x {mb / (codes + 1):>10.3f} {mb / (codes + 1) / B:>10.3f}{mark}")
    print(lines[-1], flush=True)
    if mb > ms:
        slower.append(f"batch B={B} codes={codes}")


def torch_stage(logits, dtype, mask, eos, T, pen, cur):
    x = logits.to(dtype)
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
    for B in (1, 16):
        logits = torch.randn(B, V, device=dev) * 3
        cur = torch.randint(0, V, (B, P + 150), device=dev)
        seen = lmlogits.SeenTokens(B, V, dev).mark(cur)
        out = torch.empty(B, V, device=dev)
        for dname, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            mk = mask.to(dtype)[None, :]
            for name, T, pen in (("default: mask, EOS blocked", None, 1.0), ("+ codes temperature 0.85, penalty 1.1", 0.85, 1.1)):
                f_nat = lambda: lmlogits.shape_logits(logits, None, 1.0, mask, EOS, 1, T, pen, seen, out=out, dtype=dtype)   # noqa: E731
                f_ref = lambda: torch_stage(logits, dtype, mk, EOS, T, pen, cur)                                            # noqa: E731
                for _ in range(2):
                    batch_time(f_nat, calls), batch_time(f_ref, calls)
                tn, tr = [], []
                for _ in range(runs):
                    tn.append(batch_time(f_nat, calls))
                    tr.append(batch_time(f_ref, calls))
                mn, mr = statistics.median(tn), statistics.median(tr)
                mark = "" if mn <= mr else "   **native slower**"
                lines.append(f"{B:>2} {dname:<5} {name:<40} {cell(tn, 7, 2):>26} {cell(tr, 7, 2):>28} {mr / mn:>8.2f}x{mark}")
                print(lines[-1], flush=True)
                if mn > mr:
                    slower.append(f"stage B={B} {dname} {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3, help="timed requests per side and row")
    ap.add_argument("--codes", type=int, default=150)
    ap.add_argument("--free", type=int, default=300, help="tokens of the free phase")
    ap.add_argument("--long", type=int, default=1200, help="codes of the long runs (0: skip)")
    ap.add_argument("--stage-runs", type=int, default=15)
    ap.add_argument("--stage-calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_nocfg_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from ace355 import weightgen
    from ace355.config import LmConfig
    from ace355.lm import NativeCausalLM
    cfg = LmConfig(vocab_size=V, tie_word_embeddings=True)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=0, mode="test")
    lm = NativeCausalLM(cfg, dev, max_positions=P + max(args.codes, args.long, args.free) + 16, out_dtype=torch.bfloat16)
    lm.load_state_dict(w)
    del w
    long_runs = max(1, args.runs - 1)
    lines = [f"# the 5 Hz LM without CFG, Qwen3-0.6B shape, V = {V}, out_dtype bf16, prompt {P}, {torch.cuda.get_device_name(dev)}",
             f"# top-p {TOP_P}, T {TEMP}, penalty 1, no codes temperature; whole request incl. prefill, host clock between device",
             f"# synchronisations, one warm-up request per side, then {args.runs} interleaved ({long_runs} for the long runs)",
             "# random weights only: nothing here is about a trained LM's token stream",
             "#",
             "# (a) B = 1: the native loop vs the loop before it (the reference's loop over the native forward and the native selection,",
             "#     torch operations in bf16 in between); ms per token: median [min - max]; equal: both sides drew the same tokens",
             f"{'phase':<6} {'tokens':>6}  {'native ms/token':>30} {'before ms/token':>30} {'bef / nat':>9}   {'reads':>5} {'sync-free':>9}   equal"]
    slower = []
    single_rows(lm, dev, "free", free_processor, args.free, args.runs, lines, slower)
    single_rows(lm, dev, "codes", lambda: codes_processor(args.codes), args.codes, args.runs, lines, slower)
    if args.long:
        single_rows(lm, dev, "codes", lambda: codes_processor(args.long), args.long, long_runs, lines, slower)
    lines += ["#", "# (b) B songs, one prompt, B seeds: one batched non-CFG loop vs B sequential native non-CFG loops; ms per request: median",
              "#     [min - max]; batched song i = sequential song i token for token (asserted)",
              f"{'B':>2} {'codes':>6}  {'batched ms/request':>32} {'sequential ms/request':>32} {'seq / bat':>9} {'ms/step':>10} {'ms/song-tok':>10}"]
    for B in (2, 4, 8, 16):
        batch_rows(lm, dev, B, args.codes, args.runs, lines, slower)
    if args.long:
        for B in (2, 4, 8, 16):
            batch_rows(lm, dev, B, args.long, long_runs, lines, slower)
    lm.close()
    lines += ["#", f"# (c) the stage alone, us per call (device events over {args.stage_calls} calls, {args.stage_runs} batches): shape_logits(dtype=...) vs the",
              "#     torch operations at that dtype (cast, + mask, EOS column, / T, penalty gather / where / scatter)",
              f"{'B':>2} {'dtype':<5} {'setting':<40} {'native us':>26} {'torch us':>28} {'tor / nat':>9}"]
    stage_rows(dev, args.stage_runs, args.stage_calls, lines, slower)
    lines.append("# native / batched slower at: " + (", ".join(slower) if slower else "no recorded row"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
