#!/usr/bin/env python
"""Generate g24_lm_score.npz: the reference's LM quality score (acestep/core/scoring/lm_score.py, imported by file path, like
make_g20_lyric_post.py; stub ``loguru`` / ``numba`` modules stand in where those are absent) on a fake handler.  Build container
only: it needs ``transformers``; the tests never do.

The handler (tests/_lm_score_ref.py): transformers' ``Qwen3ForCausalLM`` in fp32 on ``_lm_oracle.TINY`` weights (the ``hf_model`` recipe
of make_g21_lm.py), the toy tokenizer id <-> chr(0xE000 + id), fixed prompt strings behind ``build_formatted_prompt_for_understanding``,
a null ``_load_model_context``.

Recorded, for three (prompt, target) pairs whose targets are built greedily - the token at target column j is the model's rank-(j mod 13)
token, so ranks 0 .. 12 all occur - and for every forward of one full request (caption, lyrics, two metadata fields):
ids and prompt lengths, per-token log-probabilities (fp32, the reference's ``log_softmax``) and ranks, and the outputs of
``_calculate_log_prob``, ``_calculate_topk_recall`` and ``calculate_pmi_score_per_condition`` (scores, global score, status string).
No logits are stored.

Usage:  python tests/golden/make_g24_lm_score.py <root of the reference checkout>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ace355  # noqa: E402,F401
from ace355 import weightgen  # noqa: E402
import _lm_oracle as L  # noqa: E402
import _lm_score_ref as S  # noqa: E402
from make_g21_lm import hf_model  # noqa: E402


def import_lm_score(root: str):
    for name in ("loguru", "numba"):
        try:
            __import__(name)
        except Exception:
            m = types.ModuleType(name)
            if name == "loguru":
                m.logger = types.SimpleNamespace(**{k: (lambda *a, **kw: None) for k in ("debug", "info", "warning", "error")})
            else:
                m.jit = lambda *a, **k: (lambda f: f)
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("_ref_lm_score", os.path.join(root, "acestep", "core", "scoring", "lm_score.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def greedy_target(model, prompt_ids, T):
    """T tokens after the prompt: column j takes the token of rank j mod 13 (descending logits, equal ones by ascending id)."""
    ids = list(prompt_ids)
    with torch.no_grad():
        for j in range(T):
            logits = model(input_ids=torch.tensor([ids])).logits[0, -1].float()
            order = torch.sort(logits, descending=True, stable=True).indices
            ids.append(int(order[j % S.RANK_CYCLE]))
    return ids[len(prompt_ids):]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = import_lm_score(sys.argv[1])
    cfg, w = L.TINY, L.weights("tiny")
    model = hf_model(cfg, w)
    tok = S.ToyTokenizer(cfg.vocab_size)
    out = {"tiny_checksum": np.array(weightgen.checksum(w)), "n_pairs": np.array(len(S.PAIRS))}

    # every forward the reference makes is recorded through its own helper
    calls = []
    inner = ref._get_logits_and_target_for_scoring

    def recording(handler, prompt, target):
        logits, tids = inner(handler, prompt, target)
        if tids.shape[0]:
            lp, rank = S.token_stats(logits.float(), tids)
            full = tok(prompt + target)["input_ids"][0]
            calls.append((full.numpy().astype(np.int32), int(full.shape[0] - tids.shape[0]), lp.numpy().astype(np.float32), rank.numpy()))
        return logits, tids
    ref._get_logits_and_target_for_scoring = recording

    handler = S.FakeHandler(model, tok)
    for i, (P, T, seed) in enumerate(S.PAIRS):
        prompt = S.random_text(tok, P, seed)
        target = tok.text(greedy_target(model, tok.encode(prompt), T))
        del calls[:]
        mean_lp = ref._calculate_log_prob(handler, prompt, target)
        avg, per_k = ref._calculate_topk_recall(handler, prompt, target, topk=10)
        ids, plen, lp, rank = calls[0]
        assert plen == P and sorted(set(rank.tolist())) == list(range(min(T, S.RANK_CYCLE))), rank
        assert 0.0 < avg < 1.0
        out[f"pair{i}_ids"], out[f"pair{i}_plen"], out[f"pair{i}_lp"], out[f"pair{i}_rank"] = ids, np.array(plen), lp, rank
        out[f"pair{i}_mean_lp"], out[f"pair{i}_recall_avg"] = np.array(mean_lp), np.array(avg)
        out[f"pair{i}_recall_per_k"] = np.array([per_k[k] for k in range(1, 11)])
        print(f"pair {i}: P {P}, T {T}, mean log-prob {mean_lp:.6f}, top-10 recall {avg:.4f}", flush=True)

    rq = S.request(tok)
    handler = S.FakeHandler(model, tok, prompts=rq["prompts"])
    del calls[:]
    scores, global_score, status = ref.calculate_pmi_score_per_condition(handler, rq["audio_codes"], caption=rq["caption"],
                                                                         lyrics=rq["lyrics"], metadata=dict(rq["metadata"]))
    assert scores and "Error" not in status, status
    out["req_n_calls"] = np.array(len(calls))
    for k, (ids, plen, lp, rank) in enumerate(calls):
        out[f"req{k}_ids"], out[f"req{k}_plen"], out[f"req{k}_lp"], out[f"req{k}_rank"] = ids, np.array(plen), lp, rank
    keys = sorted(scores)
    out["req_keys"] = np.array(keys)
    out["req_scores"] = np.array([scores[k] for k in keys], dtype=np.float64)
    out["req_global"] = np.array(global_score, dtype=np.float64)
    out["req_status"] = np.array(status)
    print(f"request: {len(calls)} forwards, scores {scores}, global {global_score:.6f}\n{status}", flush=True)
    np.savez(S.G24, **out)
    print(f"{os.path.basename(S.G24)}: {os.path.getsize(S.G24)} bytes")


if __name__ == "__main__":
    main()
