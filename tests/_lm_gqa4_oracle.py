"""The configurations of the four-q-heads-per-kv-head LM tests (Qwen3-4B's 32 / 8 layout, ``allow_gqa4=True``) and fixture G25.

The forward is tests/_lm_oracle.py's composition unchanged: ``oracle.cond.encoder_layer`` repeats every kv head ``heads / kv heads``
times, whatever the ratio.  tests/golden/make_g25_lm_gqa4.py pins it against transformers at this ratio (<= G21_ORACLE_BOUND).
"""
from __future__ import annotations

import os

import numpy as np

from ace355 import weightgen
from ace355.config import LmConfig

import _lm_oracle as L

G25 = os.path.join(L.HERE, "golden", "g25_lm_gqa4.npz")

# the smallest 4 : 1 stack: two kv heads, so the q -> kv head map (hq / 4) differs from the 2 : 1 one (hq / 2) on six of eight heads
GQA4_TINY = LmConfig(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                     vocab_size=1003, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True)
# the 4B's head counts with QD = 4096 != hidden; hidden an odd multiple of 256 and intermediate an odd multiple of 64, as 2560 and
# 9728 / 8 are; a vocabulary that is no multiple of anything, untied
GQA4_WIDE = LmConfig(hidden_size=768, intermediate_size=1216, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                     vocab_size=2051, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
CONFIGS = {"gqa4_tiny": GQA4_TINY, "gqa4_wide": GQA4_WIDE}
SEEDS = {"gqa4_tiny": 25, "gqa4_wide": 26}

# acestep-5Hz-lm-4B: Qwen3-4B with the audio-code tokens
LM_4B = LmConfig(hidden_size=2560, intermediate_size=9728, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
                 vocab_size=217205, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=True)

_W = {}


def weights(name: str):
    """weightgen "test" weights under the keys of Qwen3ForCausalLM.state_dict(); made once per process and never changed."""
    if name not in _W:
        cfg = CONFIGS[name]
        _W[name] = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=SEEDS[name], mode="test")
    return _W[name]


def load_g25():
    return dict(np.load(G25))
