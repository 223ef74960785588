#!/usr/bin/env python
"""Generate g18_alignment.npz: the reference decoder's cross-attention maps for lyric alignment (build container only, like
make_golden.py, whose reference import and decoder builder it uses).

The reference's get_lyric_score runs `decoder(..., output_attentions=True, custom_layers_config=..., enable_early_exit=True,
use_cache=False)` on two rows per song: pure noise at t = 1 and t noise + (1 - t) pred at t = 1 / inference_steps
(handler/lyric_score.py:70-112).  The fixture pins that forward in fp32 (the inputs come from CPU seeds: the host's bf16 rounding of the
rows is pinned by tests/test_align_cpu.py instead) and stores the maps in the handlers' layout [n_pairs, N, L, S].

  full: the real architecture with weightgen seed-4 weights (the full_dit_seed4 fixture), SDPA self-attention as on the GPU (output_attentions
        makes cross-attention eager), T = 121 (S = 61: patch padding), L = 203; the default pairs (acestep/handler.py:129), (0, 0) / (0, 1) (two
        query heads on KV head 0) and (23, 15) from a call without early exit.
  tiny: the 2-layer tiny config, T = 41, L = 19, all four pairs.

The inputs are not stored (the full case's encoder states alone are 1.7 MB): the tests regenerate them with _xattn_capture.g18_inputs
and compare their checksums.  Each case is also run through the fp32 oracle with a capture around oracle.dit.attention
(tests/_xattn_capture.py), which must reproduce the reference within G18_ORACLE_BOUND.

Usage:  python tests/golden/make_g18_alignment.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import build_ref_decoder, import_reference_model, ref_config, to_np  # noqa: E402
from _xattn_capture import G18_ORACLE_BOUND, capture_cross, checksum, g18_inputs, g18_score_rows, handler_layout  # noqa: E402

from ace355 import align, weightgen  # noqa: E402
from oracle import dit as o_dit  # noqa: E402


def run_case(M, cfg, T, L, prs_exit, prs_full, seed, enc_seed):
    dec, o_cfg, w = build_ref_decoder(M, cfg, seed=seed)
    pred, noise, ctx, enc = g18_inputs(T, L, cfg.hidden_size, enc_seed)
    x, t = g18_score_rows(pred, noise)
    enc2, ctx2 = torch.cat([enc, enc], 0), torch.cat([ctx, ctx], 0)
    kw = dict(hidden_states=x, timestep=t, timestep_r=t, attention_mask=None, encoder_hidden_states=enc2, encoder_attention_mask=None,
              context_latents=ctx2, use_cache=False, output_attentions=True)
    layers = {}
    for l, h in prs_exit:
        layers.setdefault(l, []).append(h)
    with torch.no_grad():
        att = dec(**kw, custom_layers_config=layers, enable_early_exit=True)[2]
        att_full = dec(**kw)[2] if prs_full else None
    assert len(att) == cfg.num_hidden_layers, len(att)
    ref = [a.float() for a in att]
    if prs_full:
        ref_full = [a.float() for a in att_full]
        for l, _ in prs_exit:   # no map depends on a later layer: the early-exit call and the full call agree
            assert torch.equal(ref[l], ref_full[l]), l
    prs = list(prs_exit) + list(prs_full)
    src = [ref_full if i >= len(prs_exit) else ref for i in range(len(prs))]
    maps = torch.stack([src[i][l][:, h].transpose(-1, -2) for i, (l, h) in enumerate(prs)])
    with capture_cross(o_dit) as cap, torch.no_grad():
        o_dit.dit_forward(o_cfg, w, x, t, t, enc2, ctx2)
    om = handler_layout(cap, prs)
    d = float((om - maps).abs().max())
    print(f"  T={T} L={L} pairs={len(prs)}: |oracle - reference|max = {d:.3e} (bound {G18_ORACLE_BOUND:.0e}); "
          f"map max {float(maps.max()):.3f}, column sums within {float((maps.sum(2) - 1).abs().max()):.1e} of 1")
    assert d < G18_ORACLE_BOUND, d
    return dict(T=T, L=L, t=t, pairs=np.asarray(prs, dtype=np.int32), maps=maps, wsum=weightgen.checksum(w),
                input_sums=np.asarray(checksum(pred, noise, ctx, enc)), input_seed=enc_seed, seed=seed, oracle_maxdiff=d)


def main():
    M = import_reference_model("base")
    out = {}
    torch.manual_seed(0)
    default = align.pairs(align.DEFAULT_LAYERS_HEADS, type("C", (), {"num_hidden_layers": 24, "num_attention_heads": 16}))
    cfg = M.AceStepConfig()
    cfg._attn_implementation = "sdpa"
    print("G18 full size")
    full = run_case(M, cfg, 121, 203, [(0, 0), (0, 1)] + default, [(23, 15)], seed=4, enc_seed=180)
    out.update({f"full_{k}": v for k, v in full.items()})
    print("G18 tiny")
    tcfg = ref_config(M, attn="eager")
    tiny = run_case(M, tcfg, 41, 19, [(0, 0), (0, 1), (1, 0), (1, 1)], [], seed=2, enc_seed=181)
    out.update({f"tiny_{k}": v for k, v in tiny.items()})
    out["bound"] = G18_ORACLE_BOUND
    path = os.path.join(HERE, "g18_alignment.npz")
    np.savez_compressed(path, **to_np(out))
    print(f"G18 ok ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
