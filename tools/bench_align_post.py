#!/usr/bin/env python
"""The lyric alignment stage after the cross-attention maps: the native stage (ace355.align_post) against the host stage, on one GPU.

Shapes: a 30 s song (S = 375 frames) with L = 769 encoder rows and a 240 s song (S = 3000) with L = 2304, the lyric rows [12, L - 1),
the seven default (layer, head) pairs, host dtype bf16, timestamp (N = 1) and score (N = 2: lm and dit).  The maps are ridge maps from a
seed (the maps' own cost is in profiles/alignment_bench.txt).  Every time is the median of --reps calls, each ended by a device
synchronisation, after two warm-up calls:
  * native, per call of the C ABI: the matrix (timestamp: six kernels; score: two per item), the DTW (one launch, backtrace included; the
    score's two matrices as one batch), the metrics;
  * native, total: ace355.align_post.timestamp_spans / score_metric_values, from the fp32 maps to the per-token frame spans / the metric
    values on the host (allocations, launches, the one synchronising copy);
  * text: the Python both routes then run (timestamp: incremental token decode - quadratic in the token count, as in the reference -
    seconds, sentences, LRC lines; score: the token type mask), with the tests' toy tokenizer;
  * host: ace355.align.stack (the [layers, 16, L, S] bf16 stack) + .cpu().float() + the fp32 CPU restatement of the reference's aligners
    (tests/_lyric_post_ref.py; its DTW walks anti-diagonals in numpy - numba's compiled loop is used instead when numba imports).
--native-only skips the host stage (for a kernel trace).
Usage: python tools/bench_align_post.py [--reps 10] [--host-reps-long 3] [--native-only]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def dtw_sequential(x):
    """The column-by-column DTW loop (fp32 cost table; diagonal, up, left with strict comparisons) for numba, when it imports."""
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), 2, dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c
            trace[i, j] = t
    trace[:, 0] = 1
    trace[0, :] = 2
    rows = np.zeros(N + M, dtype=np.int32)
    cols = np.zeros(N + M, dtype=np.int32)
    i, j, k = N, M, N + M - 1
    while i > 0 or j > 0:
        rows[k], cols[k] = i - 1, j - 1
        k -= 1
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return rows[k + 1:], cols[k + 1:]


def ridge_maps_device(P, N, L, S, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    logits = torch.randn(P, N, S, L, generator=g, device=dev)
    s = torch.arange(S, device=dev, dtype=torch.float32)[:, None]
    l = torch.arange(L, device=dev, dtype=torch.float32)[None]
    logits = logits + 6.0 * torch.exp(-0.5 * ((l - s * L / S) / 1.5) ** 2)
    return torch.softmax(logits, -1).transpose(-1, -2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps-long", type=int, default=3, help="host-stage repetitions at the 240 s shape (each takes seconds)")
    ap.add_argument("--native-only", action="store_true")
    args = ap.parse_args()
    import ace355
    from ace355 import align, align_post
    import _lyric_post_ref as ref
    try:
        import numba
        host_dtw, have_numba = numba.jit(nopython=True)(dtw_sequential), True
    except Exception:
        host_dtw, have_numba = ref.dtw, False
    assert torch.cuda.is_available(), "this bench needs the GPU"
    dev = torch.device("cuda:0")
    cfg = ace355.DitConfig()
    prs = align.pairs(align.DEFAULT_LAYERS_HEADS, cfg)
    layers = {l: [h for ll, h in prs if ll == l] for l in sorted({l for l, _ in prs})}
    tok = ref.ToyTokenizer()
    print(f"# {torch.cuda.get_device_name(0)}; {len(prs)} pairs; bf16 host dtype; median of {args.reps} synchronised calls (ms); "
          f"host stage at 240 s: median of {args.host_reps_long}; numba {'imports' if have_numba else 'does not import: the host DTW is the numpy anti-diagonal restatement'}; "
          f"host CPU threads {torch.get_num_threads()}")
    print(f"{'song':>5} {'L':>5} {'S':>5} {'kind':>9} {'matrix':>8} {'dtw':>8} {'metrics':>8} {'native':>8} {'text':>8} {'host':>10} {'host/native':>11}   host = stack + copy + matrix + dtw (+ metrics), without the text")
    for secs, L, S in ((30, 769, 375), (240, 2304, 3000)):
        start, end = 12, L - 1
        R = end - start
        ids = ref.ToyTokenizer.ids(R)
        for kind, N in (("timestamp", 1), ("score", 2)):
            maps = ridge_maps_device(len(prs), N, L, S, dev, secs + N)
            if kind == "timestamp":
                calc, _ = align_post.timestamp_matrix(maps, 0, start, end, 2.0, 1, torch.bfloat16)
                t_mat = median_ms(lambda: align_post.timestamp_matrix(maps, 0, start, end, 2.0, 1, torch.bfloat16), args.reps)
                t_dtw = median_ms(lambda: align_post.dtw_raw(calc, -1.0), args.reps)
                t_met = 0.0
                t_nat = median_ms(lambda: align_post.timestamp_spans(maps, 0, start, end, torch.bfloat16), args.reps)
                spans = align_post.timestamp_spans(maps, 0, start, end, torch.bfloat16)

                def text():
                    toks = align_post.token_timestamps(tok, ids, spans, S, float(secs))
                    align_post.format_lrc(align_post.sentence_timestamps(tok, toks))
                t_text = median_ms(text, args.reps)
            else:
                mats = [align_post.score_matrix(maps, i, start, end, 1, torch.bfloat16) for i in (0, 1)]
                calc, energy = torch.stack([m[0] for m in mats]), torch.stack([m[1] for m in mats])
                path, plen, _f = align_post.dtw_raw(calc, -1.0)
                mask = torch.tensor(align_post.token_type_mask(tok, ids), dtype=torch.int32, device=dev)
                t_mat = median_ms(lambda: [align_post.score_matrix(maps, i, start, end, 1, torch.bfloat16) for i in (0, 1)], args.reps)
                t_dtw = median_ms(lambda: align_post.dtw_raw(calc, -1.0), args.reps)
                t_met = median_ms(lambda: align_post.score_metrics(energy, (path, plen), mask), args.reps)
                mask_list = mask.tolist()
                t_nat = median_ms(lambda: align_post.score_metric_values(maps, (0, 1), start, end, mask_list, torch.bfloat16), args.reps)
                t_text = median_ms(lambda: align_post.token_type_mask(tok, ids), args.reps)
            if args.native_only:
                print(f"{secs:>4}s {L:>5} {S:>5} {kind:>9} {t_mat:8.3f} {t_dtw:8.3f} {t_met:8.3f} {t_nat:8.3f} {t_text:8.3f} {'-':>10} {'-':>11}", flush=True)
                continue

            parts = {}

            def host():
                t0 = time.perf_counter()
                st = align.stack(maps, prs, 1, cfg.num_attention_heads, torch.bfloat16)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                sts = [s[:, :, start:end, :].clone().cpu().float() for s in (st if kind == "score" else [st])]
                t2 = time.perf_counter()
                t_dtw_host = 0.0
                for w in sts:
                    sel = torch.stack([w[l, h] for l, hs in layers.items() for h in hs])
                    if kind == "timestamp":
                        c, _e = ref.timestamp_matrix(sel, 2.0, 1)
                        t3 = time.perf_counter()
                        rows, cols = host_dtw(-c.astype(np.float64))
                        ref.token_frames(rows, cols, R)
                        t_dtw_host += time.perf_counter() - t3
                    else:
                        c, e = ref.score_matrix(sel, 1)
                        t3 = time.perf_counter()
                        rows, cols = host_dtw(-c.astype(np.float32))
                        t_dtw_host += time.perf_counter() - t3
                        ref.score_metrics(e, np.stack([rows, cols], 1), ref.type_mask(tok, ids))
                parts.update(stack=(t1 - t0) * 1e3, copy=(t2 - t1) * 1e3, dtw=t_dtw_host * 1e3)
            try:
                t_host = median_ms(host, args.reps if secs == 30 else args.host_reps_long, warmup=1)
                print(f"{secs:>4}s {L:>5} {S:>5} {kind:>9} {t_mat:8.3f} {t_dtw:8.3f} {t_met:8.3f} {t_nat:8.3f} {t_text:8.3f} {t_host:10.1f} {t_host / t_nat:11.1f}   "
                      f"last host call: stack {parts['stack']:.1f} copy {parts['copy']:.1f} dtw {parts['dtw']:.1f}", flush=True)
            except RuntimeError as exc:
                print(f"{secs:>4}s {L:>5} {S:>5} {kind:>9} {t_mat:8.3f} {t_dtw:8.3f} {t_met:8.3f} {t_nat:8.3f} {t_text:8.3f} {'fails':>10} {'-':>11}   "
                      f"the host stage raises: {str(exc).splitlines()[0][:120]}", flush=True)
            del maps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
