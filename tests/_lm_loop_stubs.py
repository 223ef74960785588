"""CPU stand-ins for everything the 5 Hz LM's CFG loops (``ace355.lmlogits.generate_with_cfg`` / ``generate_codes_batch``) reach on the
GPU, so that the loops' own control flow runs without one: a stub LM with seeded logits, the numpy logits stage
(tests/_lm_logits_oracle.py) behind ``shape_logits`` / ``SeenTokens``, and argmax or the fp64 selection oracle
(tests/_lm_sample_oracle.py) behind ``lmsample.pick`` / ``select_tokens``.  ``install`` puts them in place through the names the loop
looks up at call time; every stand-in appends its name to one shared log, so a test can read the order of calls."""
import numpy as np
import torch

import _lm_logits_oracle as O
import _lm_loop_ref as R
import _lm_sample_oracle as S


def role_logits(last_ids, length, seed):
    """[N, V] fp32 keyed by ``(seed, length, last id, role)``, ``role = n >= N // 2`` (conditional / unconditional): a sequence's
    logits do not depend on its row number, so song i of a batch sees what it sees alone."""
    N = len(last_ids)
    out = np.empty((N, R.V_LOOP), dtype=np.float32)
    for n, t in enumerate(last_ids):
        out[n] = np.random.default_rng([seed, length, int(t), int(n >= N // 2)]).standard_normal(R.V_LOOP).astype(np.float32) * 3
    return torch.from_numpy(out)


class StubLm:
    """What the loops ask of a ``NativeCausalLM``.  ``logits_fn(last ids, length, seed)``: ``R.fake_logits`` (G23's model) or
    ``role_logits``.  ``nan_step``: the forward of that step has a NaN at ``[0, 400]``.  ``boost``: ``(step, row, id)``, that
    forward's logit is raised by 1e4.  An id outside the vocabulary is fed as id 0, as the native embedding does."""
    out_dtype = torch.float32
    max_seqs = 16

    class cfg:
        vocab_size = R.V_LOOP

    def __init__(self, seed, log, logits_fn=R.fake_logits, nan_step=None, boost=None):
        self.seed, self.log, self.logits_fn, self.nan_step, self.boost = seed, log, logits_fn, nan_step, boost
        self.length = self.n = self.step = 0
        self.fed, self.fan_outs = [], []

    def _logits(self, last):
        x = self.logits_fn([t if 0 <= t < R.V_LOOP else 0 for t in last], self.length, self.seed)
        if self.step == self.nan_step:
            x[0, 400] = float("nan")
        if self.boost is not None and self.boost[0] == self.step:
            x[self.boost[1], self.boost[2]] += 1e4
        self.step += 1
        return x

    def prefill(self, ids, mask):
        self.log.append("prefill")
        self.n, self.length = ids.shape
        return self._logits(ids[:, -1].tolist())

    def decode_tokens(self, tokens):
        self.log.append("decode_tokens")
        t = tokens.tolist()
        self.fed.append(t)
        self.length += 1
        return self._logits([t[n % len(t)] for n in range(self.n)])

    def fan_out(self, src):
        self.log.append("fan_out")
        self.fan_outs.append(list(src))
        self.n = len(src)

    def bad_tokens(self):
        self.log.append("bad_tokens")
        return 0


class StubHandler:
    """``handler``: the tokenizer's EOS and the reference step's repetition penalty."""

    def __init__(self, eos=R.EOS):
        self.llm_tokenizer = R.FakeTokenizer(eos)

    def _build_logits_processor(self, repetition_penalty):
        if repetition_penalty == 1.0:
            return []
        return [lambda ids, scores: R.repetition_penalty(ids, scores, repetition_penalty)]


class Streamer:
    def __init__(self):
        self.put_calls, self.ended = [], 0

    def put(self, t):
        self.put_calls.append(t.clone())

    def end(self):
        self.ended += 1


def argmax_pick(x, top_k, top_p, temperature, u):
    """int64 [B]: the first maximum; -1 for a row the native selection calls bad (a NaN, a +inf, no finite entry)."""
    rows = x.numpy()
    return torch.tensor([-1 if S.is_bad(r) else int(np.argmax(r)) for r in rows], dtype=torch.int64)


def oracle_pick(x, top_k, top_p, temperature, u):
    """int64 [B]: the selection oracle row by row, with row r's uniform."""
    out = []
    for r, row in enumerate(x.numpy()):
        keep = S.keep_mask(row, top_k, top_p)
        out.append(S.greedy_token(row, keep) if u is None else S.token_for_u(row, keep, temperature, float(u[r])))
    return torch.tensor(out, dtype=torch.int64)


def install(monkeypatch, pick):
    """Replace ``lmlogits.shape_logits`` / ``SeenTokens`` and ``lmsample.pick`` / ``select_tokens``; returns the shared call log."""
    from ace355 import lmlogits, lmsample
    log = []

    class Seen:
        def __init__(self, B, V, device):
            self.B, self.V, self.ids = B, V, [[] for _ in range(B)]

        def mark(self, ids):
            log.append("mark")
            ids = ids[:, None] if ids.dim() == 1 else ids
            assert ids.shape[0] == self.B and ids.dtype == torch.int64
            for b in range(self.B):
                self.ids[b] += ids[b].tolist()
            return self

        def bitmap(self):
            n = max(len(r) for r in self.ids)
            return O.seen_bitmap(np.array([r + r[:1] * (n - len(r)) for r in self.ids]), self.V)

    def shape(cond, uncond=None, cfg_scale=1.0, mask=None, eos_id=None, eos_mode=0, temperature=None, penalty=1.0, seen=None, out=None):
        log.append("shape")
        assert mask is None or (mask.dim() == 1 and mask.dtype == torch.float32 and mask.is_contiguous())
        x = O.shape(cond.numpy(), None if uncond is None else uncond.numpy(), cfg_scale, None if mask is None else mask.numpy(), eos_id,
                    eos_mode, temperature, penalty, seen.bitmap() if penalty != 1.0 else None)
        x = torch.from_numpy(np.ascontiguousarray(x))
        return x if out is None else out.copy_(x)

    def pick_(x, top_k=None, top_p=None, temperature=1.0, u=None):
        log.append("pick")
        assert (u is not None and tuple(u.shape) == (x.shape[0],)) or not temperature > 0
        return pick(x, top_k, top_p, temperature, u if temperature > 0 else None), None, None

    def select(x, top_k=None, top_p=None, temperature=1.0, check=True):
        log.append("select")
        assert check is False
        return pick(x, top_k, top_p, temperature, torch.rand(x.shape[0]) if temperature > 0 else None)   # one global draw for all rows

    monkeypatch.setattr(lmlogits, "SeenTokens", Seen)
    monkeypatch.setattr(lmlogits, "shape_logits", shape)
    monkeypatch.setattr(lmsample, "pick", pick_)
    monkeypatch.setattr(lmsample, "select_tokens", select)
    return log
