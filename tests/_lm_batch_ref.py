"""Restatement of the reference's sequential batch path around the CFG loop - ``LLMHandler._run_pt`` (llm_inference.py:986-1070) and
the CFG branch of ``_run_pt_single`` (:826-984) - on a stub host: a tokenizer of space-separated ids, the resettable codes-phase
processor of tests/_lm_loop_ref.py, and the helper methods with the reference's signatures.  tests/test_lm_batch_gpu.py mixes
``NativeLmMixin`` over ``StubHost`` and holds the batched ``_run_pt`` to what this sequential one returns for the same seeds."""
import contextlib

import torch

import _lm_loop_ref as R


class StubTokenizer:
    """Text = ids separated by blanks.  Pads on ``padding_side`` and notes which side every batch call saw."""

    def __init__(self):
        self.eos_token_id, self.pad_token_id, self.padding_side = R.EOS, R.PAD, "right"
        self.sides = []

    def __call__(self, texts, return_tensors="pt", padding=False, truncation=True):
        assert return_tensors == "pt"
        rows = [[int(t) for t in text.split()] for text in ([texts] if isinstance(texts, str) else texts)]
        if not isinstance(texts, str):
            self.sides.append(self.padding_side)
        P = max(len(r) for r in rows)
        assert padding or all(len(r) == P for r in rows)
        left = self.padding_side == "left"
        ids = torch.tensor([[self.pad_token_id] * (P - len(r)) + r if left else r + [self.pad_token_id] * (P - len(r)) for r in rows])
        mask = torch.tensor([[0] * (P - len(r)) + [1] * len(r) if left else [1] * len(r) + [0] * (P - len(r)) for r in rows])
        return {"input_ids": ids, "attention_mask": mask}

    def decode(self, ids, skip_special_tokens=False):
        assert skip_special_tokens is False and ids.device.type == "cpu"
        return " ".join(str(int(t)) for t in ids)


class SharedProcessor(R.CodesProcessor):
    """The handler's one shared processor: ``reset`` and the setters ``_setup_constrained_processor`` calls (:291-324)."""

    def __init__(self, codes_temperature=None):
        super().__init__(R.V_LOOP, R.ALLOWED, R.EOS, codes_temperature=codes_temperature)
        self.resets = 0

    def reset(self):
        self.state, self.codes_count = R.FSMState.THINK_TAG, 0
        self.resets += 1

    def set_target_duration(self, seconds):
        self.target_codes = int(seconds * 5) if seconds is not None and seconds > 0 else None   # 5 codes = 1 second


COND_PROMPT = "11 12 13 14 7 8"      # ends with "</think>" (R.THINK_END)
UNCOND_PROMPT = "41 42 43"           # shorter: the pair's second row is left-padded


class StubHost:
    """What ``_run_pt`` needs of ``LLMHandler``.  ``calls`` counts the sequential items, ``setups`` holds what every processor setup was given."""
    offload_to_cpu = False

    def __init__(self, llm, device, codes_temperature=None):
        self.llm, self.device = llm, device
        self.llm_tokenizer = StubTokenizer()
        self.constrained_processor = SharedProcessor(codes_temperature)
        self.calls, self.contexts, self.setups = 0, 0, []

    @contextlib.contextmanager
    def _load_model_context(self):
        self.contexts += 1
        yield

    def _normalize_batch_input(self, formatted_prompts):
        is_batch = isinstance(formatted_prompts, list)
        return (formatted_prompts if is_batch else [formatted_prompts]), is_batch

    def _compute_max_new_tokens(self, target_duration, generation_phase, fallback_max=None):
        if target_duration is not None and target_duration > 0:           # (:227-246 without the GPU-tier clamp of the duration)
            return int(target_duration * 5) + (10 if generation_phase == "codes" else 500)
        return fallback_max

    def _build_logits_processor(self, repetition_penalty):
        if repetition_penalty == 1.0:
            return []
        return [lambda ids, scores: R.repetition_penalty(ids, scores, repetition_penalty)]

    def _setup_constrained_processor(self, use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata,
                                     stop_at_reasoning, skip_genres, skip_caption, skip_language, generation_phase, is_batch=False,
                                     metadata_temperature=None, codes_temperature=None):
        if not use_constrained_decoding:
            return None
        p = self.constrained_processor
        p.reset()
        p.enabled, p.debug = use_constrained_decoding, constrained_decoding_debug
        p.set_target_duration(target_duration)
        p.generation_phase = generation_phase
        self.setups.append((user_metadata, stop_at_reasoning, skip_genres, skip_caption, skip_language, is_batch))
        return p

    def _build_unconditional_prompt(self, caption, lyrics, cot_text, negative_prompt, generation_phase, is_batch=False):
        assert generation_phase == "codes" and is_batch is False
        return UNCOND_PROMPT

    def _generate_with_cfg_custom(self, *a, **k):
        raise AssertionError("the reference's own loop must not be asked")

    # ---- llm_inference.py:826-984, the cfg_scale > 1 branch
    def _run_pt_single(self, formatted_prompt, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                       use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata, stop_at_reasoning,
                       skip_genres, skip_caption, skip_language, generation_phase, caption, lyrics, cot_text):
        assert cfg_scale > 1.0
        self.calls += 1
        proc = self._setup_constrained_processor(use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata,
                                                 stop_at_reasoning, skip_genres, skip_caption, skip_language, generation_phase,
                                                 is_batch=False)
        tok = self.llm_tokenizer
        with self._load_model_context():
            max_new_tokens = self._compute_max_new_tokens(target_duration, generation_phase,
                                                          fallback_max=getattr(getattr(self.llm, "config", None), "max_new_tokens", 4096))
            uncond = self._build_unconditional_prompt(caption, lyrics, cot_text, negative_prompt, generation_phase, is_batch=False)
            side = tok.padding_side
            tok.padding_side = "left"
            pair = tok([formatted_prompt, uncond], return_tensors="pt", padding=True, truncation=True)
            tok.padding_side = side
            pair = {k: v.to(self.device) for k, v in pair.items()}
            out = self._generate_with_cfg_custom(pair["input_ids"], pair["attention_mask"], max_new_tokens, temperature, cfg_scale, top_k,
                                                 top_p, repetition_penalty, tok.pad_token_id or tok.eos_token_id, None, proc)
        new = out[0][pair["input_ids"].shape[1]:].cpu()
        return tok.decode(new, skip_special_tokens=False)

    # ---- llm_inference.py:986-1070
    def _run_pt(self, formatted_prompts, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                use_constrained_decoding=True, constrained_decoding_debug=False, target_duration=None, user_metadata=None,
                stop_at_reasoning=False, skip_genres=True, skip_caption=False, skip_language=False, generation_phase="cot", caption="",
                lyrics="", cot_text="", seeds=None):
        prompts, is_batch = self._normalize_batch_input(formatted_prompts)
        if not is_batch:
            return self._run_pt_single(prompts[0], temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                                       use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata,
                                       stop_at_reasoning, skip_genres, skip_caption, skip_language, generation_phase, caption, lyrics,
                                       cot_text)
        texts = []
        with self._load_model_context():
            for i, prompt in enumerate(prompts):
                if seeds and i < len(seeds):
                    torch.manual_seed(seeds[i])
                    torch.cuda.manual_seed_all(seeds[i])
                texts.append(self._run_pt_single(prompt, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                                                 use_constrained_decoding, constrained_decoding_debug, target_duration, None, False, True,
                                                 True, True, generation_phase, caption, lyrics, cot_text))
        return texts


def make_handler(llm, device, codes_temperature=None, batch=True):
    """``NativeLmMixin`` over ``StubHost`` with the native loop on (the sequential path's yardstick) and the batched path as asked."""
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, StubHost):
        pass

    h = Handler(llm, device, codes_temperature)
    h.use_native_lm_loop, h.use_native_lm_batch = True, batch
    return h

