"""Shared pieces of the LM-score tests and of tests/golden/make_g24_lm_score.py: a toy tokenizer, a fake ``LLMHandler``, the fixed request
of fixture G24, and the per-token statistics (log-probability, rank) of a logits matrix.

The tokenizer is a bijection on the ids it is built for: id <-> ``chr(0xE000 + id)`` (the private-use area, which ``yaml.dump(...,
allow_unicode=True)`` leaves alone).  The fixed ASCII the reference wraps around a target (``<think>``, ``caption: `` ...) falls outside
that range and maps to ``ord(ch) % vocab``: many-to-one, which is all a scoring test needs of it.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
G24 = os.path.join(HERE, "golden", "g24_lm_score.npz")
BASE = 0xE000
RANK_CYCLE = 13   # target column j holds the model's rank-(j mod 13) token: ranks 0 .. 12, so top-10 recall is neither 0 nor 1

# (prompt tokens, target tokens, seed) of the three recorded pairs
PAIRS = [(17, 13, 2401), (33, 26, 2402), (48, 31, 2403)]
REQUEST_SEED = 2410


class Encoding(dict):
    """What ``tokenizer(...)`` returns, as far as the scoring code uses it: a dict with ``.to(device)``."""

    def to(self, device):
        return Encoding({k: v.to(device) for k, v in self.items()})


class ToyTokenizer:
    def __init__(self, vocab: int):
        self.vocab = int(vocab)

    def encode(self, text: str):
        return [(ord(ch) - BASE) if BASE <= ord(ch) < BASE + self.vocab else ord(ch) % self.vocab for ch in text]

    def text(self, ids) -> str:
        return "".join(chr(BASE + int(i)) for i in ids)

    def __call__(self, text, return_tensors="pt", padding=False, truncation=False, add_special_tokens=True):
        ids = torch.tensor([self.encode(text)], dtype=torch.int64)
        return Encoding(input_ids=ids, attention_mask=torch.ones_like(ids))


class FakeHandler:
    """The attributes and methods lm_score.py (and ace355.lmscore) touch on an ``LLMHandler``."""

    llm_initialized = True
    llm_backend = "pt"
    use_native_lm_score = False

    def __init__(self, llm, tokenizer, device="cpu", prompts=None):
        self.llm, self.llm_tokenizer, self.device = llm, tokenizer, device
        self.prompts = prompts or {}
        self.context_entries = 0

    def get_hf_model_for_scoring(self):
        return self.llm

    @contextlib.contextmanager
    def _load_model_context(self):
        self.context_entries += 1
        yield

    def build_formatted_prompt_for_understanding(self, audio_codes, is_negative_prompt=False):
        return self.prompts["uncond" if audio_codes == "NO USER INPUT" else "cond"]


def random_text(tok: ToyTokenizer, n: int, seed: int) -> str:
    g = torch.Generator().manual_seed(seed)
    return tok.text(torch.randint(0, tok.vocab, (n,), generator=g).tolist())


def request(tok: ToyTokenizer) -> dict:
    """G24's full request: prompts, audio codes, caption, lyrics and two metadata fields."""
    s = REQUEST_SEED
    return {"prompts": {"cond": random_text(tok, 41, s), "uncond": random_text(tok, 29, s + 1)},
            "audio_codes": "<|audio_code_1|><|audio_code_2|>",
            "caption": random_text(tok, 11, s + 2), "lyrics": random_text(tok, 19, s + 3),
            "metadata": {"bpm": 120, "keyscale": random_text(tok, 3, s + 4)}}


def token_stats(logits: torch.Tensor, targets: torch.Tensor):
    """Per row of ``logits`` [T, V] and its target: ``(log_softmax(logits)[t], 0-based rank of t)``, the rank counting ids with a
    larger logit, or an equal one and a lower id.  In the dtype of ``logits``."""
    t = targets.long()
    rows = torch.arange(t.shape[0])
    lp = torch.log_softmax(logits, dim=-1)[rows, t]
    z = logits[rows, t][:, None]
    ids = torch.arange(logits.shape[1])[None, :]
    rank = ((logits > z) | ((logits == z) & (ids < t[:, None]))).sum(1)
    return lp, rank.to(torch.int32)


def load_g24() -> dict:
    return dict(np.load(G24, allow_pickle=False))
