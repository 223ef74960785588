#!/usr/bin/env python
"""Generate the G19 fixture: transformers' Qwen3Model (the reference's text encoder, Qwen3-Embedding-0.6B, loaded with
AutoModel.from_pretrained in init_service_loader.py:146-161) in fp32 with eager attention, on weightgen "test" weights.  Build
container only, like make_g18_alignment.py: it needs `transformers`; the tests never do.

The reference calls the encoder as `text_encoder(input_ids=ids, lyric_attention_mask=None)` (conditioning_embed.py:71-79): right-padded
ids, no attention mask, so every row - pad rows included - is a purely causal function of the padded sequence.  The same cases run through
the oracle composition (tests/_textenc_oracle.py), which must reproduce transformers within G19_ORACLE_BOUND, and through that composition
in the oracle's bf16-storage mode: per sequence, the relative L2 of that run against fp32 is the drift the GPU gates are twice of.

  tiny a: hidden 256, 2 layers, 4 q / 2 kv heads of 128, vocab 1003; B = 3, lengths (37, 20, 1), pad id 1002.
  tiny b: same model, B = 2, S = 300 (several key tiles; S not a multiple of 64), no padding.
  full:   the published 0.6B shape (hidden 1024, 28 layers, 16 / 8 heads, vocab 151669); B = 3, lengths (256, 131, 7), pad id 151643.

Files: g19_text_encoder.npz (ids, tiny outputs, checksums, per-sequence norms and drifts) and g19_text_encoder_full_part{0..3}.npz (the
full case's fp32 outputs, 192 rows each: no committed file may exceed 1 MiB).

Usage:  python tests/golden/make_g19_text_encoder.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ace355  # noqa: E402,F401
from ace355 import weightgen  # noqa: E402
from ace355.config import TextEncoderConfig  # noqa: E402
from oracle import dit as o_dit  # noqa: E402
import _textenc_oracle as T  # noqa: E402


def hf_model(cfg: TextEncoderConfig, w):
    from transformers import Qwen3Config, Qwen3Model
    c = Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                    rope_theta=cfg.rope_theta, max_position_embeddings=4096, attention_bias=False, use_sliding_window=False,
                    tie_word_embeddings=True)
    c._attn_implementation = "eager"
    assert TextEncoderConfig.from_reference(c) == cfg, (TextEncoderConfig.from_reference(c), cfg)
    m = Qwen3Model(c).eval()
    missing, unexpected = m.load_state_dict(w, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return m


def run_case(name, cfg, w, ids, out):
    with torch.no_grad():
        ref = hf_model(cfg, w)(input_ids=ids, lyric_attention_mask=None).last_hidden_state.float()
        orc = T.text_encoder(cfg, w, ids)
        with o_dit.bf16_storage():
            emu = T.text_encoder(cfg, o_dit.bf16_weights(w), ids)
    bound = T.rel(orc, ref)
    assert bound <= T.G19_ORACLE_BOUND, f"{name}: oracle vs transformers {bound:.3e}"
    drift = np.array([T.rel(emu[b], ref[b]) for b in range(ids.shape[0])])
    norm = np.array([float(ref[b].double().norm()) for b in range(ids.shape[0])])
    print(f"{name}: ids {tuple(ids.shape)}, oracle vs transformers {bound:.2e}, bf16-storage drift per sequence {np.round(drift, 5)}, "
          f"whole tensor {T.rel(emu, ref):.3e}", flush=True)
    out[f"{name}_ids"] = ids.numpy().astype(np.int32)
    out[f"{name}_drift"] = drift
    out[f"{name}_drift_all"] = np.array(T.rel(emu, ref))
    out[f"{name}_norm"] = norm
    return ref


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    wt = T.weights(T.TINY, T.TINY_SEED)
    out["tiny_checksum"] = np.array(weightgen.checksum(wt))
    out["tiny_a_out"] = run_case("tiny_a", T.TINY, wt, T.padded_ids((37, 20, 1), 37, T.TINY.vocab_size, T.TINY_PAD, 1), out).numpy()
    out["tiny_b_out"] = run_case("tiny_b", T.TINY, wt, T.padded_ids((300, 300), 300, T.TINY.vocab_size, T.TINY_PAD, 2), out).numpy()
    del wt
    wf = T.weights(T.FULL, T.FULL_SEED)
    out["full_checksum"] = np.array(weightgen.checksum(wf))
    full = run_case("full", T.FULL, wf, T.padded_ids((256, 131, 7), 256, T.FULL.vocab_size, T.FULL_PAD, 3), out).numpy()
    np.savez(T.G19, **out)
    rows = full.reshape(-1, T.FULL.hidden_size).astype(np.float32)
    for k, p in enumerate(T.G19_FULL_PARTS):
        np.savez(p, rows=rows[k * 192:(k + 1) * 192])
    for p in [T.G19] + T.G19_FULL_PARTS:
        print(f"{os.path.basename(p)}: {os.path.getsize(p)} bytes")


if __name__ == "__main__":
    main()
