"""The text encoder (transformers' Qwen3Model, the reference's Qwen3-Embedding-0.6B) composed from the oracle's existing pieces, and the
G19 fixture's configurations.

Qwen3Model = embed_tokens -> num_hidden_layers pre-norm decoder layers -> RMSNorm, and a Qwen3 decoder layer is
``oracle.cond.encoder_layer`` (q / k head norms, RoPE, GQA, SwiGLU, plain residuals) with a causal mask.  The reference passes no attention
mask (conditioning_embed.py:71-79), so the mask is ``tril`` over the padded length for every sequence.  tests/golden/make_g19_text_encoder.py
pins this composition against transformers (<= G19_ORACLE_BOUND relative, measured 0.0 on the eager path).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ace355 import weightgen
from ace355.config import TextEncoderConfig
from oracle import cond as o_cond
from oracle import dit as o_dit

HERE = os.path.dirname(os.path.abspath(__file__))
G19 = os.path.join(HERE, "golden", "g19_text_encoder.npz")
# the full case's fp32 outputs [3, 256, 1024] in four files of 192 rows each (no committed file may exceed 1 MiB)
G19_FULL_PARTS = [os.path.join(HERE, "golden", f"g19_text_encoder_full_part{k}.npz") for k in range(4)]
G19_ORACLE_BOUND = 1e-5

TINY = TextEncoderConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                         head_dim=128, vocab_size=1003, rms_norm_eps=1e-6, rope_theta=1e6)
FULL = TextEncoderConfig(hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8,
                         head_dim=128, vocab_size=151669, rms_norm_eps=1e-6, rope_theta=1e6)
TINY_SEED, FULL_SEED = 19, 190
TINY_PAD, FULL_PAD = 1002, 151643   # the tiny vocabulary's last id; Qwen's <|endoftext|> pad token


def weights(cfg: TextEncoderConfig, seed: int):
    return weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=seed, mode="test")


def padded_ids(lengths, S, vocab, pad, seed):
    """Right-padded random caption ids [len(lengths), S] (ids drawn from [0, vocab - 1) so that the pad id stands out)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), S), pad, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = torch.randint(0, vocab - 1, (n,), generator=g)
    return ids


def _ocfg(cfg: TextEncoderConfig) -> o_cond.CondConfig:
    return o_cond.CondConfig(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_attention_heads=cfg.num_attention_heads,
                             num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                             rope_theta=cfg.rope_theta, num_lyric_encoder_hidden_layers=cfg.num_hidden_layers,
                             num_timbre_encoder_hidden_layers=0)


def text_encoder(cfg: TextEncoderConfig, w, ids: torch.Tensor) -> torch.Tensor:
    """Qwen3Model(input_ids=ids).last_hidden_state in fp32 (or in the oracle's bf16-storage mode, see tests/_drift.py)."""
    oc = _ocfg(cfg)
    S = ids.shape[1]
    x = w["embed_tokens.weight"][ids.long()].float()
    cos, sin = o_dit.rope_cos_sin(S, cfg.head_dim, cfg.rope_theta)
    mask = o_dit.additive_mask(torch.tril(torch.ones(S, S, dtype=torch.bool)))[None, None]
    for li in range(cfg.num_hidden_layers):
        x = o_cond.encoder_layer(oc, w, f"layers.{li}.", x, cos, sin, mask)
    return o_dit.rms_norm(x, w["norm.weight"], cfg.rms_norm_eps)


def rel(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def load_g19():
    z = dict(np.load(G19))
    if all(os.path.exists(p) for p in G19_FULL_PARTS):
        z["full_out"] = np.concatenate([np.load(p)["rows"] for p in G19_FULL_PARTS], 0).reshape(z["full_ids"].shape + (FULL.hidden_size,))
    return z
