"""The 5 Hz LM's forward (transformers' Qwen3ForCausalLM) composed from the oracle's existing pieces, and the G21 fixture's configurations.

Qwen3ForCausalLM = the text encoder's stack (tests/_textenc_oracle.py: embed_tokens -> pre-norm decoder layers = ``oracle.cond.encoder_layer``
-> RMSNorm) + ``lm_head``.  The reference's CFG loop sends left-padded batches with a ``0...0 1...1`` mask and no ``position_ids``
(llm_inference.py:2414-2533), so the token in column j has RoPE position j and the query in column i of sequence n sees keys
``first[n] <= j <= i``: the mask here is ``tril & (j >= first[n])``.  Only the last column's logits are consumed.

The oracle needs no cache: the logits of decode step t are a full recompute over ``ids[:, :P + t]`` - or, the stack being causal,
column ``P + t - 1`` of one pass over a longer run (``lm_logits_at``).
tests/golden/make_g21_lm.py pins this composition against transformers run WITH its cache (<= G21_ORACLE_BOUND relative).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ace355 import weightgen
from ace355.config import LmConfig
from oracle import cond as o_cond
from oracle import dit as o_dit

from _textenc_oracle import _ocfg, rel  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
G21 = os.path.join(HERE, "golden", "g21_lm.npz")
G21_ORACLE_BOUND = 1e-5

_TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
             vocab_size=1003, rms_norm_eps=1e-6, rope_theta=1e6)
TINY = LmConfig(**_TINY, tie_word_embeddings=True)
TINY_UNTIED = LmConfig(**_TINY, tie_word_embeddings=False)
# QD = 16 x 128 = 2048 != hidden, as in the 0.6B, and 8 kv heads for the decode grid; a vocabulary that is no multiple of anything
WIDE = LmConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8, head_dim=128,
                vocab_size=2051, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
CONFIGS = {"tiny": TINY, "tiny_untied": TINY_UNTIED, "wide": WIDE}
SEEDS = {"tiny": 21, "tiny_untied": 22, "wide": 23}


def weights(name: str):
    """weightgen "test" weights under the keys of Qwen3ForCausalLM.state_dict() (a tied set has no lm_head.weight)."""
    cfg = CONFIGS[name]
    return weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=SEEDS[name], mode="test")


def left_padded(lengths, P, vocab, seed, pad=0):
    """ids [len(lengths), P] with lengths[n] random tokens at the right end, and first[n] = P - lengths[n]; the pad columns hold `pad`."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lengths), P), pad, dtype=torch.int64)
    for n, L in enumerate(lengths):
        ids[n, P - L:] = torch.randint(0, vocab, (L,), generator=g)
    return ids, [P - L for L in lengths]


def mask_of(first, P) -> torch.Tensor:
    """The reference's attention_mask [N, P]: zeros below first[n], ones from there on."""
    return (torch.arange(P)[None, :] >= torch.tensor(first)[:, None]).long()


def lm_logits_at(cfg: LmConfig, w, ids: torch.Tensor, first, cols) -> torch.Tensor:
    """Qwen3ForCausalLM(input_ids=ids, attention_mask=mask_of(first)).logits[:, cols, :] in fp32 (or in the oracle's bf16-storage mode,
    see tests/_drift.py): [N, len(cols), V].  The stack is causal, so column c of a run over ids equals the last column of a run over
    ids[:, :c + 1]: one pass over the whole length gives every decode step's logits without a cache."""
    oc = _ocfg(cfg)
    N, S = ids.shape
    x = w["model.embed_tokens.weight"][ids.long()].float()
    cos, sin = o_dit.rope_cos_sin(S, cfg.head_dim, cfg.rope_theta)
    j = torch.arange(S)
    valid = torch.tril(torch.ones(S, S, dtype=torch.bool))[None] & (j[None, None, :] >= torch.as_tensor(first).view(N, 1, 1))
    mask = o_dit.additive_mask(valid)[:, None]
    for li in range(cfg.num_hidden_layers):
        x = o_cond.encoder_layer(oc, w, f"model.layers.{li}.", x, cos, sin, mask)
    last = o_dit.rms_norm(x[:, list(cols), :], w["model.norm.weight"], cfg.rms_norm_eps)
    head = w["model.embed_tokens.weight"] if cfg.tie_word_embeddings else w["lm_head.weight"]
    return o_dit._linear(last, head)


def lm_logits(cfg: LmConfig, w, ids: torch.Tensor, first) -> torch.Tensor:
    """The last column's logits [N, V]: what the reference reads after every step."""
    return lm_logits_at(cfg, w, ids, first, [ids.shape[1] - 1])[:, 0]


def teacher_forced(cfg: LmConfig, w, ids: torch.Tensor, first, P: int, fn=lm_logits):
    """[lm_logits over ids[:, :P + t] for t = 0 .. ids.shape[1] - P]: step 0 is the prefill, step t the decode step that was fed
    ids[:, P + t - 1]."""
    return [fn(cfg, w, ids[:, :P + t], first) for t in range(ids.shape[1] - P + 1)]


def load_g21():
    return dict(np.load(G21))
