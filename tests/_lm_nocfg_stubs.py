"""CPU stand-ins for everything the 5 Hz LM's non-CFG loops (``ace355.lmlogits.generate_constrained`` /
``generate_codes_batch_nocfg``) reach on the GPU, modelled on tests/_lm_loop_stubs.py: a stub LM with seeded logits and an
``out_dtype``, the numpy logits stage at either dtype (tests/_lm_nocfg_oracle.py, tests/_lm_logits_oracle.py) behind the dtype-aware
``shape_logits`` / ``SeenTokens``, and argmax or the fp64 selection oracle behind ``lmsample.pick`` / ``select_tokens``.  ``install``
puts them in place through the names the loop looks up at call time; every stand-in appends its name to one shared log."""
import numpy as np
import torch

import _lm_logits_oracle as O
import _lm_loop_ref as R
import _lm_loop_stubs as St
import _lm_nocfg_oracle as N

StubHandler, Streamer, argmax_pick, oracle_pick = St.StubHandler, St.Streamer, St.argmax_pick, St.oracle_pick


def song_logits(last_ids, length, seed):
    """[N, V] fp32 keyed by ``(seed, length, last id)`` alone: a sequence's logits do not depend on its row number, so song i of a
    batch sees what it sees alone.  The EOS logit does not rise: only a target ends these loops."""
    out = np.empty((len(last_ids), R.V_LOOP), dtype=np.float32)
    for n, t in enumerate(last_ids):
        out[n] = np.random.default_rng([seed, length, int(t)]).standard_normal(R.V_LOOP).astype(np.float32) * 3
    return torch.from_numpy(out)


class StubLm(St.StubLm):
    """``_lm_loop_stubs.StubLm`` with the model's output dtype.  The forward's logits stay fp32, as the native forward's do."""

    def __init__(self, seed, log, out_dtype, logits_fn=R.fake_logits, nan_step=None, boost=None, max_seqs=16):
        super().__init__(seed, log, logits_fn, nan_step, boost)
        self.out_dtype, self.max_seqs = out_dtype, max_seqs


def unique_argmax_pick(x, top_k, top_p, temperature, u):
    """``_lm_loop_stubs.argmax_pick`` that refuses a tied maximum (G26's greedy steps have none)."""
    for r in x.numpy():
        assert (r == r.max()).sum() == 1 or np.isnan(r).any()
    return St.argmax_pick(x, top_k, top_p, temperature, u)


def install(monkeypatch, pick):
    """Replace ``lmlogits.shape_logits`` / ``SeenTokens`` and ``lmsample.pick`` / ``select_tokens``; returns ``(log, shapes)``: the
    shared call log and the ``(dtype, rows, has uncond)`` of every stage call."""
    from ace355 import lmlogits, lmsample
    log = St.install(monkeypatch, pick)          # SeenTokens, pick, select_tokens as the CFG loops' stubs have them
    old_shape = lmlogits.shape_logits            # (the old signature: what the two CFG modes must keep calling)
    shapes = []

    def shape(cond, uncond=None, cfg_scale=1.0, mask=None, eos_id=None, eos_mode=0, temperature=None, penalty=1.0, seen=None, out=None,
              dtype=None):
        shapes.append((dtype, cond.shape[0], uncond is not None))
        if dtype in (None, torch.float32):
            return old_shape(cond, uncond, cfg_scale, mask, eos_id, eos_mode, temperature, penalty, seen, out)
        assert dtype == torch.bfloat16 and uncond is None and cond.dtype == torch.float32
        log.append("shape")
        assert mask is None or (mask.dim() == 1 and mask.dtype == torch.float32 and mask.is_contiguous())
        x = N.shape(cond.numpy(), None if mask is None else mask.numpy(), eos_id, eos_mode, temperature, penalty,
                    seen.bitmap() if penalty != 1.0 else None)
        x = torch.from_numpy(np.ascontiguousarray(x))
        return x if out is None else out.copy_(x)

    monkeypatch.setattr(lmlogits, "shape_logits", shape)
    return log, shapes
