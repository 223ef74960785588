#!/usr/bin/env python
"""Native text encoder vs transformers' Qwen3Model (bf16, same weights, same GPU) -> profiles/text_encoder_bench.txt.

The published Qwen3-Embedding-0.6B shape with weightgen "test" weights.  Caption shapes (B, S) = (1, 64), (1, 256), (8, 256), (16, 256):
the reference's right-padded caption batches; plus embed_tokens on [8, 2048] lyric ids.  Each side is warmed up, then the two run
interleaved (native, PyTorch, native, ...) and every call is timed on its own with device events around it; the table gives the median and
the spread (min - max) over the runs.  The native call starts from host int32 ids (the library uploads them, as the seam passes them);
the PyTorch call gets ids already on the device.  Without `transformers` the native side is measured alone and the file says so.

Usage:  python tools/bench_text_encoder.py [--runs 30] [--out profiles/text_encoder_bench.txt]
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
from ace355 import weightgen  # noqa: E402
from ace355.config import TextEncoderConfig  # noqa: E402
from ace355.textenc import NativeTextEncoder  # noqa: E402

SHAPES = [(1, 64), (1, 256), (8, 256), (16, 256)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def hf_model(cfg, w, dev):
    try:
        from transformers import Qwen3Config, Qwen3Model
    except Exception as exc:  # noqa: BLE001
        return None, f"transformers does not import here ({type(exc).__name__}: {exc}); native only"
    c = Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                    rope_theta=cfg.rope_theta, max_position_embeddings=32768, use_sliding_window=False)
    m = Qwen3Model(c)
    m.load_state_dict(w, strict=False)
    import transformers
    return m.to(dev, torch.bfloat16).eval(), f"transformers {transformers.__version__}, attn_implementation {c._attn_implementation}"


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = TextEncoderConfig()
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=0, mode="test")
    nat = NativeTextEncoder(cfg, dev)
    nat.load_state_dict(w)
    ref, note = hf_model(cfg, w, dev)
    del w
    g = torch.Generator().manual_seed(0)
    lines = [f"# native text encoder vs PyTorch, Qwen3-Embedding-0.6B shape ({cfg.num_hidden_layers} layers, hidden {cfg.hidden_size}), "
             f"{torch.cuda.get_device_name(dev)}", f"# {note}",
             f"# {args.warmup} warm-up calls per side, then {args.runs} interleaved runs; ms per call: median [min - max]",
             f"{'call':<24} {'native ms':>26} {'pytorch ms':>26} {'pytorch / native':>17}"]
    cases = [(f"encode B={B} S={S}", torch.randint(0, cfg.vocab_size, (B, S), generator=g), "encode") for B, S in SHAPES]
    cases.append(("embed_tokens [8, 2048]", torch.randint(0, cfg.vocab_size, (8, 2048), generator=g), "embed"))
    with torch.inference_mode():
        for name, ids, kind in cases:
            ids_dev = ids.to(dev)
            if kind == "encode":
                f_nat = lambda: nat(ids)  # noqa: E731
                f_ref = (lambda: ref(input_ids=ids_dev).last_hidden_state) if ref is not None else None  # noqa: E731
            else:
                f_nat = lambda: nat.embed_tokens(ids)  # noqa: E731
                f_ref = (lambda: ref.embed_tokens(ids_dev)) if ref is not None else None  # noqa: E731
            for _ in range(args.warmup):
                f_nat()
                if f_ref:
                    f_ref()
            torch.cuda.synchronize()
            tn, tr = [], []
            for _ in range(args.runs):
                tn.append(timed(f_nat))
                if f_ref:
                    tr.append(timed(f_ref))
            mn = stats(tn)
            cell_n = f"{mn[0]:8.3f} [{mn[1]:.3f} - {mn[2]:.3f}]"
            if tr:
                mr = stats(tr)
                cell_r, ratio = f"{mr[0]:8.3f} [{mr[1]:.3f} - {mr[2]:.3f}]", f"{mr[0] / mn[0]:.2f}x"
            else:
                cell_r, ratio = "-", "-"
            lines.append(f"{name:<24} {cell_n:>26} {cell_r:>26} {ratio:>17}")
            print(lines[-1], flush=True)
    nat.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
