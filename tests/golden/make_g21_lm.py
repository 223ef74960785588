#!/usr/bin/env python
"""Generate the G21 fixture: transformers' Qwen3ForCausalLM (the reference's 5 Hz LM) in fp32 with eager attention, on weightgen "test"
weights, driven the way the reference's CFG loop drives it (llm_inference.py:2414-2533): a left-padded batch with a `0...0 1...1` mask and
no position_ids, `use_cache=True` for the prefill, then teacher-forced one-token steps that carry `past_key_values` and a mask grown by a
column of ones.  Build container only, like make_g19_text_encoder.py: it needs `transformers`; the tests never do.

  wide:  hidden 512, 2 layers, 16 q / 8 kv heads of 128, vocab 2051, untied head; N = 3, P = 70, first = (0, 5, 69); prefill + 4 steps.
         Recorded: ids, first, the last column's logits of every step, the weight checksum, and per step the drift of the oracle
         composition (tests/_lm_oracle.py, a full recompute without a cache) in its bf16-storage mode against transformers.
         The fp32 composition must reproduce transformers (with its cache) within G21_ORACLE_BOUND.
  seam:  the tiny tied model, a CFG pair (N = 2, prompts of 23 and 9 tokens, left-padded to P = 23), 8 greedy steps of the oracle.
         The token seed is the first one for which, at all 8 steps, the oracle's top-1 / top-2 logit gap exceeds 4 x the bf16-storage
         emulation's largest absolute logit error (so the emulation alone picks the oracle's tokens); ids and seed are recorded.

Usage:  python tests/golden/make_g21_lm.py
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
from ace355.config import LmConfig  # noqa: E402
import _drift  # noqa: E402
import _lm_oracle as L  # noqa: E402

WIDE_P, WIDE_STEPS, WIDE_LENGTHS = 70, 4, (70, 65, 1)
SEAM_P, SEAM_STEPS, SEAM_LENGTHS = 23, 8, (23, 9)


def hf_model(cfg: LmConfig, w):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    c = Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                    num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                    num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, rms_norm_eps=cfg.rms_norm_eps,
                    rope_theta=cfg.rope_theta, max_position_embeddings=4096, attention_bias=False, use_sliding_window=False,
                    tie_word_embeddings=cfg.tie_word_embeddings)
    c._attn_implementation = "eager"
    assert LmConfig.from_reference(c) == cfg, (LmConfig.from_reference(c), cfg)
    m = Qwen3ForCausalLM(c).eval()
    missing, unexpected = m.load_state_dict(w, strict=False)
    assert not unexpected and all("rotary" in k or (cfg.tie_word_embeddings and k == "lm_head.weight") for k in missing), (missing, unexpected)
    if cfg.tie_word_embeddings:
        m.tie_weights()
    return m


def hf_steps(model, ids, first, P):
    """The reference's loop: prefill over ids[:, :P], then one teacher-forced token per step with the returned cache."""
    out, past = [], None
    with torch.no_grad():
        for t in range(ids.shape[1] - P + 1):
            mask = L.mask_of(first, P + t)
            if t == 0:
                o = model(input_ids=ids[:, :P], attention_mask=mask, use_cache=True)
            else:
                o = model(input_ids=ids[:, P + t - 1:P + t], past_key_values=past, attention_mask=mask, use_cache=True)
            past = o.past_key_values
            out.append(o.logits[:, -1, :].float())
    return out


def seam_case(cfg, w, seed):
    """Greedy continuation of a left-padded CFG pair by the fp32 oracle; per step the top-1 / top-2 gap and the emulation's error."""
    ids, first = L.left_padded(SEAM_LENGTHS, SEAM_P, cfg.vocab_size, seed)
    ok = []
    for _t in range(SEAM_STEPS):
        ref = L.lm_logits(cfg, w, ids, first)
        emu = _drift.emulated(L.lm_logits, cfg, w, ids, first)
        top2 = ref.topk(2, dim=-1).values
        ok.append(float((top2[:, 0] - top2[:, 1]).min()) > 4.0 * float((emu - ref).abs().max()))
        ids = torch.cat([ids, ref.argmax(-1, keepdim=True)], 1)
    return ids, first, ok


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    cfg, w = L.WIDE, L.weights("wide")
    out["wide_checksum"] = np.array(weightgen.checksum(w))
    ids, first = L.left_padded(WIDE_LENGTHS, WIDE_P, cfg.vocab_size, 210)
    g = torch.Generator().manual_seed(211)
    ids = torch.cat([ids, torch.randint(0, cfg.vocab_size, (ids.shape[0], WIDE_STEPS), generator=g)], 1)
    ref = hf_steps(hf_model(cfg, w), ids, first, WIDE_P)
    with torch.no_grad():
        orc = L.teacher_forced(cfg, w, ids, first, WIDE_P)
        emu = L.teacher_forced(cfg, w, ids, first, WIDE_P, fn=lambda c, w_, i, f: _drift.emulated(L.lm_logits, c, w_, i, f))
    for t, (r, o) in enumerate(zip(ref, orc)):
        bound = L.rel(o, r)
        assert bound <= L.G21_ORACLE_BOUND, f"wide step {t}: oracle vs transformers {bound:.3e}"
        print(f"wide step {t}: oracle vs transformers {bound:.2e}, bf16-storage drift per sequence "
              f"{[round(L.rel(emu[t][n], r[n]), 5) for n in range(ids.shape[0])]}, whole {L.rel(emu[t], r):.3e}", flush=True)
    out["wide_ids"] = ids.numpy().astype(np.int32)
    out["wide_first"] = np.array(first, dtype=np.int32)
    out["wide_P"] = np.array(WIDE_P)
    out["wide_logits"] = torch.stack(ref).numpy().astype(np.float32)                                   # [steps + 1, N, V]
    out["wide_drift"] = np.array([[L.rel(e[n], r[n]) for n in range(ids.shape[0])] for e, r in zip(emu, ref)])
    out["wide_drift_all"] = np.array([L.rel(e, r) for e, r in zip(emu, ref)])

    cfg, w = L.TINY, L.weights("tiny")
    out["tiny_checksum"] = np.array(weightgen.checksum(w))
    with torch.no_grad():
        for seed in range(1000):
            sids, sfirst, ok = seam_case(cfg, w, seed)
            if all(ok):
                break
        else:
            raise SystemExit("no token seed qualifies on all 8 steps")
        href = hf_steps(hf_model(cfg, w), sids[:, :-1], sfirst, SEAM_P)
        for t, r in enumerate(href):
            b = L.rel(L.lm_logits(cfg, w, sids[:, :SEAM_P + t], sfirst), r)
            assert b <= L.G21_ORACLE_BOUND, f"seam step {t}: oracle vs transformers {b:.3e}"
            assert torch.equal(r.argmax(-1), sids[:, SEAM_P + t]), f"seam step {t}: transformers picks other tokens"
    print(f"seam: token seed {seed} qualifies on all {SEAM_STEPS} steps; ids {tuple(sids.shape)}, first {sfirst}", flush=True)
    out["seam_seed"] = np.array(seed)
    out["seam_ids"] = sids.numpy().astype(np.int32)     # [2, P + 8]: the prompts and the 8 greedy tokens
    out["seam_first"] = np.array(sfirst, dtype=np.int32)
    out["seam_P"] = np.array(SEAM_P)
    np.savez(L.G21, **out)
    print(f"{os.path.basename(L.G21)}: {os.path.getsize(L.G21)} bytes")


if __name__ == "__main__":
    main()
