#!/usr/bin/env python
"""Generate the G25 fixture: G21's "wide" recipe (make_g21_lm.py) on a stack with FOUR q heads per kv head, Qwen3-4B's layout.

transformers' Qwen3ForCausalLM in fp32 with eager attention, on weightgen "test" weights, driven as the reference's CFG loop drives it: a
left-padded batch with a `0...0 1...1` mask and no position_ids, `use_cache=True` for the prefill, then teacher-forced one-token steps
that carry `past_key_values`.  Build container only: it needs `transformers`; the tests never do.

  gqa4_wide (tests/_lm_gqa4_oracle.py): hidden 768, intermediate 1216, 2 layers, 32 q / 8 kv heads of 128, vocab 2051, untied head;
         N = 3, P = 70, first = (0, 5, 69); prefill + 4 steps.  Recorded: ids, first, the last column's logits of every step, the weight
         checksum, and per step and sequence the drift of the oracle composition (tests/_lm_oracle.py) in its bf16-storage mode against
         transformers.  The fp32 composition must reproduce transformers (with its cache) within G21_ORACLE_BOUND.

Usage:  python tests/golden/make_g25_lm_gqa4.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ace355  # noqa: E402,F401
from ace355 import weightgen  # noqa: E402
from ace355.config import LmConfig  # noqa: E402
import _drift  # noqa: E402
import _lm_gqa4_oracle as Q  # noqa: E402
import _lm_oracle as L  # noqa: E402
from make_g21_lm import WIDE_LENGTHS, WIDE_P, WIDE_STEPS, hf_steps  # noqa: E402

NAME = "gqa4_wide"


def hf_model(cfg: LmConfig, w):
    """make_g21_lm.hf_model with the opt-in that the 4 : 1 layout needs."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                    rope_theta=cfg.rope_theta, max_position_embeddings=4096, attention_bias=False, use_sliding_window=False,
                    tie_word_embeddings=cfg.tie_word_embeddings)
    c._attn_implementation = "eager"
    assert LmConfig.from_reference(c, allow_gqa4=True) == cfg, (LmConfig.from_reference(c, allow_gqa4=True), cfg)
    m = Qwen3ForCausalLM(c).eval()
    missing, unexpected = m.load_state_dict(w, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return m


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg, w = Q.CONFIGS[NAME], Q.weights(NAME)
    out = {"checksum": np.array(weightgen.checksum(w))}
    ids, first = L.left_padded(WIDE_LENGTHS, WIDE_P, cfg.vocab_size, 250)
    g = torch.Generator().manual_seed(251)
    ids = torch.cat([ids, torch.randint(0, cfg.vocab_size, (ids.shape[0], WIDE_STEPS), generator=g)], 1)
    ref = hf_steps(hf_model(cfg, w), ids, first, WIDE_P)
    with torch.no_grad():
        orc = L.teacher_forced(cfg, w, ids, first, WIDE_P)
        emu = L.teacher_forced(cfg, w, ids, first, WIDE_P, fn=lambda c, w_, i, f: _drift.emulated(L.lm_logits, c, w_, i, f))
    for t, (r, o) in enumerate(zip(ref, orc)):
        bound = L.rel(o, r)
        assert bound <= L.G21_ORACLE_BOUND, f"step {t}: oracle vs transformers {bound:.3e}"
        print(f"step {t}: oracle vs transformers {bound:.2e}, bf16-storage drift per sequence "
              f"{[round(L.rel(emu[t][n], r[n]), 5) for n in range(ids.shape[0])]}, whole {L.rel(emu[t], r):.3e}", flush=True)
    out["ids"] = ids.numpy().astype(np.int32)
    out["first"] = np.array(first, dtype=np.int32)
    out["P"] = np.array(WIDE_P)
    out["logits"] = torch.stack(ref).numpy().astype(np.float32)                                   # [steps + 1, N, V]
    out["drift"] = np.array([[L.rel(e[n], r[n]) for n in range(ids.shape[0])] for e, r in zip(emu, ref)])
    out["drift_all"] = np.array([L.rel(e, r) for e, r in zip(emu, ref)])
    np.savez(Q.G25, **out)
    print(f"{os.path.basename(Q.G25)}: {os.path.getsize(Q.G25)} bytes")


if __name__ == "__main__":
    main()
