#!/usr/bin/env python
"""Native 5 Hz LM forward vs transformers' Qwen3ForCausalLM (bf16, same weights, same GPU) -> profiles/lm_step_bench.txt.

The Qwen3-0.6B shape (28 layers, hidden 1024, 16 / 8 heads, tied head, vocabulary 151669 + 65536 audio-code tokens stand-ins) with
weightgen "test" weights.  For (N, length) in (2, 512), (2, 2048), (16, 512), (16, 2048): one prefill of [N, length] left-padded ids
(the second half of the batch carries 64 pad columns, as a CFG batch's unconditional prompts do) and the decode steps that follow it,
each side driven as LLMHandler._forward_pass drives the model (mask grown by a column per step, the previous call's cache handed
back).  Each side is warmed up, then the two run interleaved (native, PyTorch, native, ...) and every call is timed on its own with
device events around it; the table gives the median and the spread (min - max) over the runs.  Decode runs advance the cache, so a row
covers lengths length .. length + runs.  No hipGraph on either side.

The byte floor of a decode step is what it must read once: every layer's weights and the head (bf16), plus the K / V rows of the
cache, N x kv heads x length x 128 x 2 x 2 bytes per layer, over the chip's measured HBM copy bandwidth (6.3 TB/s; 8.0 TB/s on paper).

--model 4b: the Qwen3-4B shape (36 layers, hidden 2560, intermediate 9728, 32 / 8 heads, tied head, the same vocabulary) on a handle
created with ``allow_gqa4=True`` -> profiles/lm_gqa4_bench.txt.  The PyTorch side is then built on the GPU in bf16 (an fp32 host copy
of 4 B parameters beside the weights' own would be 32 GB).

Usage:  python tools/bench_lm.py [--model {0.6b,4b}] [--runs 20] [--out profiles/lm_step_bench.txt]
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
from ace355 import native, weightgen  # noqa: E402
from ace355.config import LmConfig  # noqa: E402
from ace355.lm import NativeCausalLM  # noqa: E402

SHAPES = [(2, 512), (2, 2048), (16, 512), (16, 2048)]
HBM_BYTES_PER_S = 6.3e12
PADS = 64
VOCAB = 151669 + 65536
MODELS = {"0.6b": dict(name="Qwen3-0.6B", cfg=dict(), out="lm_step_bench.txt"),
          "4b": dict(name="Qwen3-4B", cfg=dict(hidden_size=2560, intermediate_size=9728, num_hidden_layers=36, num_attention_heads=32,
                                               num_key_value_heads=8), out="lm_gqa4_bench.txt")}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def hf_model(cfg, w, dev, on_device=False):
    try:
        import transformers
        from transformers import Qwen3Config, Qwen3ForCausalLM
    except Exception as exc:  # noqa: BLE001
        return None, f"transformers does not import here ({type(exc).__name__}: {exc}); native only"
    c = Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                    rope_theta=cfg.rope_theta, max_position_embeddings=32768, use_sliding_window=False,
                    tie_word_embeddings=cfg.tie_word_embeddings)
    if on_device:
        dtype = torch.get_default_dtype()
        torch.set_default_dtype(torch.bfloat16)
        try:
            with torch.device(dev):
                m = Qwen3ForCausalLM(c)
        finally:
            torch.set_default_dtype(dtype)
    else:
        m = Qwen3ForCausalLM(c)
    m.load_state_dict(w, strict=False)
    if cfg.tie_word_embeddings:
        m.tie_weights()
    return m.to(dev, torch.bfloat16).eval(), f"transformers {transformers.__version__}, attn_implementation {c._attn_implementation}"


def step_floor_bytes(cfg, N, length):
    D, F, QD, KVD = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    layer_w = 2 * ((QD + 2 * KVD) * D + D * QD + 2 * F * D + D * F)
    kv = N * cfg.num_key_value_heads * length * 128 * 2 * 2
    return cfg.num_hidden_layers * (layer_w + kv) + 2 * cfg.vocab_size * D


def step_launches(cfg, N, length):
    """Kernel launches of one native decode step: the pass plan's calls (the decode attention is two kernels, the cut and its merge),
    the embedding gather ahead of the stack and the LM head behind it."""
    p = native.encoder_pass_plan(cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                                 cfg.num_hidden_layers, N, 1, causal=1, has_cache=1, pos0=length - 1, max_pos=length, max_seqs=N, has_first=1)
    return sum(p["calls"].values()) + p["calls"]["decode_attn"] + 2


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def cell(xs):
    m = stats(xs)
    return f"{m[0]:8.3f} [{m[1]:.3f} - {m[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20, help="decode steps timed per side and shape")
    ap.add_argument("--prefill-runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", choices=sorted(MODELS), default="0.6b")
    ap.add_argument("--out", default=None, help="default: profiles/lm_step_bench.txt (0.6b), profiles/lm_gqa4_bench.txt (4b)")
    ap.add_argument("--no-pytorch", action="store_true", help="time the native side alone")
    args = ap.parse_args()
    model = MODELS[args.model]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", model["out"])
    dev = torch.device("cuda:0")
    cfg = LmConfig(vocab_size=VOCAB, tie_word_embeddings=True, **model["cfg"])
    gqa4 = cfg.num_attention_heads == 4 * cfg.num_key_value_heads
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=0, mode="test")
    opt_in = {"allow_gqa4": True} if gqa4 else {}
    nat = NativeCausalLM(cfg, dev, max_positions=max(L for _n, L in SHAPES) + args.runs + args.warmup + 8, out_dtype=torch.bfloat16, **opt_in)
    nat.load_state_dict(w)
    ref, note = (None, "PyTorch side not run (--no-pytorch)") if args.no_pytorch else hf_model(cfg, w, dev, on_device=gqa4)
    del w
    g = torch.Generator().manual_seed(0)
    lines = [f"# native LM forward vs PyTorch, {model['name']} shape ({cfg.num_hidden_layers} layers, hidden {cfg.hidden_size}, vocabulary "
             f"{cfg.vocab_size}, tied head), {torch.cuda.get_device_name(dev)}", f"# {note}",
             f"# {args.warmup} warm-up calls per side, then interleaved runs ({args.prefill_runs} prefills, {args.runs} decode steps); "
             "ms per call: median [min - max]",
             f"# byte floor of a decode step: layer weights + head + K / V rows read once, over {HBM_BYTES_PER_S / 1e12:.1f} TB/s",
             *([f"# {cfg.num_attention_heads} / {cfg.num_key_value_heads} heads: 4 q heads per kv head (allow_gqa4); kernel launches per "
                f"native decode step: {step_launches(cfg, 16, 2048)} (per layer 2 norms, 4 GEMMs, K / V store, decode attention + merge; "
                "embedding gather, final norm, LM head)"] if gqa4 else []),
             f"{'call':<26} {'native ms':>26} {'pytorch ms':>26} {'pytorch / native':>17} {'floor ms':>9} {'floor MB':>9}"]
    slower = []
    with torch.inference_mode():
        for N, P in SHAPES:
            ids = torch.randint(0, cfg.vocab_size, (N, P), generator=g).to(dev)
            mask = torch.ones(N, P, dtype=torch.long, device=dev)
            mask[N // 2:, :PADS] = 0
            nxt = torch.randint(0, cfg.vocab_size, (N, 1), generator=g).to(dev)
            f_nat = lambda: nat(input_ids=ids, attention_mask=mask, use_cache=True)  # noqa: E731
            f_ref = (lambda: ref(input_ids=ids, attention_mask=mask, use_cache=True)) if ref is not None else None  # noqa: E731
            for _ in range(args.warmup):
                f_nat()
                if f_ref:
                    f_ref()
            torch.cuda.synchronize()
            tn, tr = [], []
            for _ in range(args.prefill_runs):
                tn.append(timed(f_nat))
                if f_ref:
                    tr.append(timed(f_ref))
            rows = [(f"prefill N={N} P={P}", tn, tr, None)]
            # decode: both sides continue their last prefill, one token per step
            state = {"n": f_nat().past_key_values, "r": f_ref().past_key_values if f_ref else None, "mask": mask}

            def step_nat():
                state["n"] = nat(input_ids=nxt, past_key_values=state["n"], attention_mask=state["mask"], use_cache=True).past_key_values

            def step_ref():
                state["r"] = ref(input_ids=nxt, past_key_values=state["r"], attention_mask=state["mask"], use_cache=True).past_key_values

            tn, tr = [], []
            for i in range(args.warmup + args.runs):
                state["mask"] = torch.cat([state["mask"], torch.ones(N, 1, dtype=torch.long, device=dev)], 1)
                a = timed(step_nat)
                b = timed(step_ref) if f_ref else None
                if i >= args.warmup:
                    tn.append(a)
                    if f_ref:
                        tr.append(b)
            rows.append((f"decode N={N} length={P}", tn, tr, step_floor_bytes(cfg, N, P)))
            for name, a, b, floor in rows:
                ratio = f"{stats(b)[0] / stats(a)[0]:.2f}x" if b else "-"
                fl = (f"{floor / HBM_BYTES_PER_S * 1e3:9.3f}", f"{floor / 1e6:9.1f}") if floor else ("-", "-")
                lines.append(f"{name:<26} {cell(a):>26} {(cell(b) if b else '-'):>26} {ratio:>17} {fl[0]:>9} {fl[1]:>9}")
                print(lines[-1], flush=True)
                if b and stats(a)[0] > stats(b)[0]:
                    slower.append(name)
            state.clear()
            torch.cuda.empty_cache()
    lines.append("# native slower than PyTorch at: " + (", ".join(slower) if slower else "no recorded shape"))
    nat.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
