#!/usr/bin/env python
"""Generate g22_lm_sample.npz: what the reference's own token-selection methods keep (build container only, like
make_g20_lyric_post.py).

``LLMHandler`` is imported from the reference on the CPU (``loguru`` is absent here, so a stub module whose ``logger`` swallows every
call stands in) and its ``_apply_top_k_filter``, ``_apply_top_p_filter`` and ``_sample_tokens`` are called unbound, in that order, as its
loops call them.  Per case the file holds the input logits, and per setting ``k``, ``p``, ``isfinite`` of the filtered logits (bit-packed)
and the greedy token.  Arrays only.

Cases: V in {1, 2, 63, 64, 65, 1003, 2051} with 3 rows of seeded ``randn * 3`` each; a codes-phase row (a contiguous id range plus one
separate "EOS" id finite, the rest -inf); a forced-EOS row (one finite entry); a row with planted duplicates exactly at the k-th value; a
peaked row whose first mass exceeds p; a row with fewer finite entries than k.  Settings per case: (k off, p 0.9), (k = min(50, V // 2),
p off), (k, p 0.95), both off.

What this pins: on every recorded row the prefix masses of the top-p walk stay at least 1e-3 away from p and the values either side of
the cut differ, so the kept set does not depend on the reference's fp32 cumsum (off by about 1.2e-4 at worst over 2051 terms) nor on how
``torch.sort`` orders equal values; the script asserts that, asserts that the reference's kept set equals the fp64 restatement's
(tests/_lm_sample_oracle.py), and re-draws the seed of a row that does not qualify.  Everything is random logits; nothing here says
anything about a trained LM's token stream.

Usage:  python tests/golden/make_g22_lm_sample.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _lm_sample_oracle as O  # noqa: E402

REF = "/root/reference"
MARGIN = 1e-3
SEED0 = 2200


def import_handler():
    class _Quiet:
        def __getattr__(self, name):
            return lambda *a, **k: self

    lg = types.ModuleType("loguru")
    lg.logger = _Quiet()
    sys.modules.setdefault("loguru", lg)
    sys.path.insert(0, REF)
    from acestep.llm_inference import LLMHandler
    return LLMHandler


def settings(V):
    k = min(50, V // 2)
    return [(0, 0.9), (k, 0.0), (k, 0.95), (0, 0.0)]


def randn_row(V, seed):
    return (torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 3).numpy()


def make_row(kind, V, seed):
    x = randn_row(V, seed)
    if kind == "codes":       # the codes phase: audio-code ids [300, 900) and one EOS id
        y = np.full(V, -np.inf, dtype=np.float32)
        y[300:900] = x[300:900]
        y[2000] = x[2000]
        return y
    if kind == "eos":         # a forced EOS: one finite entry
        y = np.full(V, -np.inf, dtype=np.float32)
        y[777] = x[777]
        return y
    if kind == "dup":         # four more entries exactly at the k-th value (k = 50), planted over the four smallest
        t = np.sort(x)[::-1][49]
        x[np.argsort(x)[:4]] = t
        return x
    if kind == "peaked":      # the first mass alone exceeds p
        x[7] = 40.0
        return x
    if kind == "few":         # fewer finite entries than k
        y = np.full(V, -np.inf, dtype=np.float32)
        keep = np.random.default_rng(seed).choice(V, 20, replace=False)
        y[keep] = x[keep]
        return y
    return x


def qualifies(x, V):
    for k, p in settings(V):
        dist, differ = O.top_p_margin(x, k or None, p or None)
        if dist < MARGIN or not differ:
            return False
    return True


def main():
    H = import_handler()
    cases = [("randn", V, 3) for V in (1, 2, 63, 64, 65, 1003, 2051)]
    cases += [("codes", 2051, 1), ("eos", 1003, 1), ("dup", 1003, 1), ("peaked", 1003, 1), ("few", 1003, 1)]
    out = {"n_cases": np.int64(len(cases)), "margin": np.float64(MARGIN)}
    seed = SEED0
    for c, (kind, V, R) in enumerate(cases):
        rows = []
        for _r in range(R):
            while True:
                seed += 1
                x = make_row(kind, V, seed)
                if qualifies(x, V):
                    break
                print("case", c, kind, "seed", seed, "re-drawn")
            rows.append(x)
        x = np.stack(rows).astype(np.float32)
        out[f"c{c}_x"] = x
        out[f"c{c}_kind"] = np.array(kind)
        out[f"c{c}_k"] = np.array([k for k, _p in settings(V)], dtype=np.int32)
        out[f"c{c}_p"] = np.array([p for _k, p in settings(V)], dtype=np.float64)
        for s, (k, p) in enumerate(settings(V)):
            t = torch.from_numpy(x.copy())
            t = H._apply_top_k_filter(None, t, k)
            t = H._apply_top_p_filter(None, t, p)
            fin = torch.isfinite(t).numpy()
            greedy = H._sample_tokens(None, t, 0.0).numpy().astype(np.int64)
            for r in range(R):
                keep = O.keep_mask(x[r], k or None, p or None)
                assert (keep == fin[r]).all(), (c, kind, s, r, int(keep.sum()), int(fin[r].sum()))
                assert O.greedy_token(x[r], keep) == int(greedy[r]), (c, kind, s, r)
            out[f"c{c}_s{s}_finite"] = np.packbits(fin, axis=1)
            out[f"c{c}_s{s}_greedy"] = greedy
            print(c, kind, V, "k", k, "p", p, "kept", fin.sum(1).tolist(), "greedy", greedy.tolist())
    dst = os.path.join(HERE, "g22_lm_sample.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
