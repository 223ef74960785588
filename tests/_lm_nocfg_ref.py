"""Restatement of the reference's non-CFG loop (``LLMHandler._generate_with_constrained_decoding``, llm_inference.py:2321-2412) with
the forward, the logits stage and the token selection as callables, and the CPU fake model behind G26's loop cases.  The processor
branches it needs are those of tests/_lm_loop_ref.py's ``CodesProcessor`` (disabled, ``COMPLETED`` with the "understand" mask,
``CODES_GENERATION``).  G26 records what the reference's real loop returned; tests/test_lm_nocfg_cpu.py holds this file to it, and
tests/test_lm_nocfg_gpu.py then drives it with the native forward as the yardstick for the native loop.
"""
import os
import types

import numpy as np
import torch

import _lm_loop_ref as R

G26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_lm_nocfg.npz")
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
PHASES = ("understand", "target", "free", "disabled", "none")
MAX_NEW = 12


def torch_stage(dtype, penalty):
    """The reference's torch operations between forward and selection (llm_inference.py:2369-2377) in the model's ``dtype``, on
    whatever device the logits are: no upcast anywhere."""
    def stage(logits, cur_ids, processor):
        x = logits.to(dtype)
        if processor is not None:
            x = processor(cur_ids, x)
        if penalty != 1.0:
            x = R.repetition_penalty(cur_ids, x, penalty)
        return x
    return stage


def run_loop(forward, stage, select, input_ids, max_new_tokens, eos_token_id, pad_token_id, processor=None, streamer=None):
    """``forward(generated_ids [B, L], step) -> logits [B, V]``; ``stage(logits, ids [B, L], processor) -> [B, V]``;
    ``select([B, V]) -> int64 [B]``.  Returns the ids [B, P + steps]."""
    generated = input_ids.clone()
    for step in range(max_new_tokens):
        x = stage(forward(generated, step), generated, processor)
        tokens = select(x)
        host = tokens.tolist()
        if processor is not None:
            for t in host:                      # _update_constrained_processor_state: once per row
                processor.update_state(t)
        stop = eos_token_id in host or (pad_token_id is not None and pad_token_id != eos_token_id and pad_token_id in host)
        generated = torch.cat([generated, tokens.to(generated.dtype).unsqueeze(1)], dim=1)
        if streamer is not None:
            streamer.put(tokens.unsqueeze(1))
        if stop:
            break
    if streamer is not None:
        streamer.end()
    return generated


class FakeModel(R.FakeModel):
    """``_lm_loop_ref.FakeModel`` with logits in the case's dtype, as a bf16 model returns them."""

    def __init__(self, seed, dtype):
        super().__init__(seed)
        self.dtype = dtype

    def __call__(self, **kw):
        out = super().__call__(**kw)
        return types.SimpleNamespace(logits=out.logits.to(self.dtype), past_key_values=out.past_key_values)


def forward_of(model):
    """``run_loop``'s forward on a ``FakeModel``."""
    def forward(g, step):
        return model(input_ids=g if step == 0 else g[:, -1:], attention_mask=torch.ones(g.shape),
                     past_key_values=None if step == 0 else 1).logits[:, 0]
    return forward


def loop_cases():
    """(name, dtype name, B, phase, penalty, codes temperature, base seed)"""
    out = []
    for dt in DTYPES:
        for B in (1, 2):
            for phase in PHASES:
                for pen, T in ((1.0, None), (1.3, 0.85)):
                    out.append((f"{dt}_B{B}_{phase}_p{pen}", dt, B, phase, pen, T, 2600 + len(out)))
    return out


def loop_prompt(B):
    """ids and mask [B, 6]: the conditional rows of ``_lm_loop_ref.loop_prompt`` (the second one left-padded)."""
    ids, am = R.loop_prompt(B)
    return ids[:B].clone(), am[:B].clone()


def make_processor(phase, T):
    """The processor of a phase as the reference's loop meets it, or None.  "understand": the metadata is done (``COMPLETED``) and
    the free-form text runs under the ``audio_code_mask`` (-inf on the audio codes) until EOS."""
    if phase == "none":
        return None
    p = R.CodesProcessor(R.V_LOOP, R.ALLOWED, R.EOS, target_codes=6 if phase == "target" else None, codes_temperature=T,
                         metadata_temperature=T, generation_phase="understand" if phase == "understand" else "codes",
                         enabled=phase != "disabled")
    m = torch.zeros(1, R.V_LOOP)
    m[0, list(R.ALLOWED)] = float("-inf")
    p.audio_code_mask = m
    if phase == "understand":
        p.state = R.FSMState.COMPLETED
    return p


def unique_argmax(x):
    """argmax of [B, V], asserting that every row's maximum is unique: a greedy step that no tie-break decides."""
    x = x.float()
    top = x.max(dim=-1, keepdim=True).values
    assert bool(((x == top).sum(dim=-1) == 1).all()), "a greedy step with a tied maximum"
    return torch.argmax(x, dim=-1)


def load_g26_loop():
    """name -> (ids, final state name or "", count or -1, the seed the script settled on)."""
    z = np.load(G26)
    return {c[0]: (z[f"l_{c[0]}_ids"], str(z[f"l_{c[0]}_state"]), int(z[f"l_{c[0]}_count"]), int(z[f"l_{c[0]}_seed"])) for c in loop_cases()}
