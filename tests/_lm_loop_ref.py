"""Restatement of the reference's CFG loop (``LLMHandler._generate_with_cfg_custom``, llm_inference.py:2414-2533) with the forward, the
logits stage and the token selection as callables, the branches of its constrained processor that the codes phase takes, and the CPU
fake model behind G23's loop cases.  G23 records what the reference's real loop returned; tests/test_lm_logits_cpu.py holds this file
to it, and tests/test_lm_logits_gpu.py then drives it with the native forward as the yardstick for the native loop.
"""
import enum
import os
import types

import numpy as np
import torch

G23 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_lm_logits.npz")
THINK_END = [7, 8]   # what the fake tokenizer makes of "</think>"


class FSMState(enum.Enum):
    THINK_TAG = 1
    CODES_GENERATION = 2
    COMPLETED = 3


class FakeTokenizer:
    def __init__(self, eos_token_id):
        self.eos_token_id = eos_token_id

    def encode(self, text, add_special_tokens=False):
        assert text == "</think>"
        return list(THINK_END)


class CodesProcessor:
    """``MetadataConstrainedLogitsProcessor`` as far as a codes-phase request exercises it: ``__call__`` for a disabled processor,
    ``COMPLETED``, the ``THINK_TAG -> CODES_GENERATION`` jump and ``CODES_GENERATION`` (constrained_logits_processor.py:1583-1629),
    ``_apply_temperature_scaling`` (:1666-1695) and ``update_state``'s first three branches (:2147-2158).  Any other state raises."""

    def __init__(self, V, allowed, eos_token_id, target_codes=None, codes_temperature=None, metadata_temperature=None,
                 generation_phase="codes", enabled=True):
        self.enabled = enabled
        self.state = FSMState.THINK_TAG
        self.generation_phase = generation_phase
        self.tokenizer = FakeTokenizer(eos_token_id)
        self.eos_token_id = eos_token_id
        self.target_codes = target_codes
        self.codes_count = 0
        self.codes_temperature = codes_temperature
        self.metadata_temperature = metadata_temperature
        self.debug = False
        self.user_field_token_queue = []
        m = torch.full((1, V), float("-inf"))
        m[0, list(allowed)] = 0
        m[0, eos_token_id] = 0
        self.non_audio_code_mask = m     # [1, V], as _build_audio_code_mask leaves it
        self.audio_code_mask = None

    def _apply_temperature_scaling(self, scores):
        T = self.codes_temperature if self.state in (FSMState.CODES_GENERATION, FSMState.COMPLETED) else self.metadata_temperature
        if T is None:
            return scores
        if T <= 0:
            T = 1e-6
        return scores / T

    def _input_contains_think_end_tag(self, input_ids):
        n = len(THINK_END)
        for b in range(input_ids.shape[0]):
            seq = input_ids[b].tolist()
            if any(seq[i:i + n] == THINK_END for i in range(len(seq) - n + 1)):
                return True
        return False

    def __call__(self, input_ids, scores):
        if not self.enabled:
            return self._apply_temperature_scaling(scores)
        if self.state == FSMState.COMPLETED:
            if self.generation_phase == "understand" and self.audio_code_mask is not None:
                if self.audio_code_mask.device != scores.device or self.audio_code_mask.dtype != scores.dtype:
                    self.audio_code_mask = self.audio_code_mask.to(device=scores.device, dtype=scores.dtype)
                scores = scores + self.audio_code_mask
            return self._apply_temperature_scaling(scores)
        if self.generation_phase == "codes" and self.state == FSMState.THINK_TAG and self._input_contains_think_end_tag(input_ids):
            self.state = FSMState.CODES_GENERATION
            self.codes_count = 0
        if self.state != FSMState.CODES_GENERATION:
            raise NotImplementedError("the metadata FSM is not restated here")
        if self.non_audio_code_mask is not None:
            if self.non_audio_code_mask.device != scores.device or self.non_audio_code_mask.dtype != scores.dtype:
                self.non_audio_code_mask = self.non_audio_code_mask.to(device=scores.device, dtype=scores.dtype)
            scores = scores + self.non_audio_code_mask
        if self.target_codes is not None and self.eos_token_id is not None:
            if self.codes_count < self.target_codes:
                scores[:, self.eos_token_id] = float("-inf")
            else:
                eos_scores = scores[:, self.eos_token_id].clone()
                scores.fill_(float("-inf"))
                scores[:, self.eos_token_id] = eos_scores
        return self._apply_temperature_scaling(scores)

    def update_state(self, generated_token_id):
        if not self.enabled or self.state == FSMState.COMPLETED:
            return
        if self.state == FSMState.CODES_GENERATION:
            self.codes_count += 1
            return
        raise NotImplementedError("the metadata FSM is not restated here")


def repetition_penalty(input_ids, scores, penalty):
    """transformers' RepetitionPenaltyLogitsProcessor.__call__ for 2-D scores: gather, where, scatter."""
    score = torch.gather(scores, 1, input_ids)
    score = torch.where(score < 0, score * penalty, score / penalty)
    return scores.scatter(1, input_ids, score)


def torch_stage(cfg_scale, penalty):
    """The reference's torch operations between forward and selection (llm_inference.py:2482-2493), on whatever device the logits are."""
    def stage(cond, uncond, cur_ids, processor):
        x = uncond.float() + cfg_scale * (cond.float() - uncond.float())
        if processor is not None:
            x = processor(cur_ids, x)
        if penalty != 1.0:
            x = repetition_penalty(cur_ids, x, penalty)
        return x
    return stage


def run_loop(forward, stage, select, batch_input_ids, max_new_tokens, eos_token_id, pad_token_id, processor=None, streamer=None):
    """``forward(generated_ids [2B, L], step) -> logits [2B, V]``; ``stage(cond, uncond, cond ids [B, L], processor) -> [B, V]``;
    ``select([B, V]) -> int64 [B]``.  Returns the ids [2B, P + steps], conditional rows first."""
    B = batch_input_ids.shape[0] // 2
    generated = batch_input_ids.clone()
    for step in range(max_new_tokens):
        logits = forward(generated, step)
        x = stage(logits[:B], logits[B:], generated[:B], processor)
        tokens = select(x)
        host = tokens.tolist()
        if processor is not None:
            for t in host:                      # _update_constrained_processor_state: once per row
                processor.update_state(t)
        stop = eos_token_id in host or (pad_token_id is not None and pad_token_id != eos_token_id and pad_token_id in host)
        generated = torch.cat([generated, tokens.to(generated.dtype).unsqueeze(1).repeat(2, 1)], dim=1)
        if streamer is not None:
            streamer.put(tokens.unsqueeze(1))
        if stop:
            break
    if streamer is not None:
        streamer.end()
    return generated


# ------------------------------------------------------------------ G23's loop cases
V_LOOP, EOS, PAD, ALLOWED, MAX_NEW = 1003, 950, 951, range(300, 900), 12
CFG_SCALE = 2.0


def fake_logits(last_ids, length, seed):
    """[N, V] fp32: a seeded function of every row's last id and of the mask length; the EOS logit rises with the length so that a
    loop without a target stops by itself."""
    out = np.empty((len(last_ids), V_LOOP), dtype=np.float32)
    for n, t in enumerate(last_ids):
        out[n] = np.random.default_rng([seed, length, int(t), n]).standard_normal(V_LOOP).astype(np.float32) * 3
    out[:, EOS] += np.float32(6.0 * (length - 7))
    return torch.from_numpy(out)


class FakeModel:
    """What ``_forward_pass`` needs of ``Qwen3ForCausalLM`` (llm_inference.py:416-438)."""

    def __init__(self, seed):
        self.seed = seed
        self.generation_config = types.SimpleNamespace(use_cache=True)
        self.calls = 0

    def __call__(self, input_ids=None, attention_mask=None, past_key_values=None, use_cache=True):
        assert (past_key_values is None) == (self.calls == 0) and (past_key_values is not None) == (input_ids.shape[1] == 1)
        self.calls += 1
        logits = fake_logits(input_ids[:, -1].tolist(), attention_mask.shape[1], self.seed)
        return types.SimpleNamespace(logits=logits[:, None, :], past_key_values=("kv", self.calls))


def loop_cases():
    """(name, B, target_codes, penalty, codes temperature, seed)"""
    out = []
    for B in (1, 2):
        for target in (6, None):
            for pen, T in ((1.0, None), (1.3, 0.85)):
                out.append((f"B{B}_t{target}_p{pen}", B, target, pen, T, 2300 + len(out)))
    return out


def loop_prompt(B):
    """ids and mask [2B, 6]: "</think>" ends every conditional row; the second pair of rows is left-padded."""
    rows = [[11, 12, 13, 14] + THINK_END, [PAD, PAD, 21, 22] + THINK_END][:B]
    un = [[31, 32, 33, 34, 35, 36], [PAD, PAD, PAD, 41, 42, 43]][:B]
    ids = torch.tensor(rows + un, dtype=torch.int64)
    return ids, (ids != PAD).long()


def make_processor(target, T):
    return CodesProcessor(V_LOOP, ALLOWED, EOS, target_codes=target, codes_temperature=T)


def load_g23_loop():
    z = np.load(G23)
    return {name: (z[f"l_{name}_ids"], str(z[f"l_{name}_state"]), int(z[f"l_{name}_count"])) for name, *_ in loop_cases()}
