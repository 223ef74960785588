#!/usr/bin/env python
"""Generate g23_lm_logits.npz: what the reference's own logits stage and CFG loop compute (build container only, like
make_g22_lm_sample.py).

``LLMHandler`` and ``MetadataConstrainedLogitsProcessor`` are imported from the reference on the CPU (``loguru`` is absent here, so a
stub module whose ``logger`` swallows every call stands in) and their methods are called unbound on plain namespaces that carry only the
attributes those methods read.  Arrays only.

(a) Stage cases, V in {1, 31, 32, 33, 65, 1003, 2051}, B = 3: seeded ``randn * 3`` conditional and unconditional logits, a codes mask
(0 on about half the ids and on the EOS id, -inf elsewhere), an "understand" mask, a history of 9 ids per row with a duplicate and two
pad ids.  Per setting (processor branch, temperature none / 0.7 / 0, penalty 1 / 1.1 / 1.3; cfg_scale 1.7) the file holds the output of
``uncond + cfg_scale * (cond - uncond)`` -> ``MetadataConstrainedLogitsProcessor.__call__`` -> the list ``_build_logits_processor``
returns.  The small V take all 54 settings, V = 1003 takes 24, V = 2051 one per branch.  The V = 65 case has planted signed zeros, the
V = 33 case an id where both logits are -inf (NaN out).  The script asserts that tests/_lm_logits_oracle.py gives the same bits.

(b) Loop cases: the reference's real ``_generate_with_cfg_custom`` on tests/_lm_loop_ref.py's CPU fake model, greedy, B = 1 and 2,
target 6 codes and no target (EOS reachable), penalty / codes temperature off and 1.3 / 0.85.  The processor is the reference's
``__call__`` / ``update_state`` / ``_apply_temperature_scaling`` / ``_input_contains_think_end_tag`` on a namespace.  Per case: the
returned ids and the processor's final state and count.  The script asserts that tests/_lm_loop_ref.py reproduces each.

Everything is random logits; nothing here says anything about a trained LM's token stream.

Usage:  python tests/golden/make_g23_lm_logits.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _lm_logits_oracle as O  # noqa: E402
import _lm_loop_ref as L  # noqa: E402

REF = "/root/reference"
SEED0 = 2300


def import_reference():
    class _Quiet:
        def __getattr__(self, name):
            return lambda *a, **k: self

    lg = types.ModuleType("loguru")
    lg.logger = _Quiet()
    sys.modules.setdefault("loguru", lg)
    sys.path.insert(0, REF)
    from acestep.llm_inference import LLMHandler
    from acestep.constrained_logits_processor import FSMState, MetadataConstrainedLogitsProcessor
    return LLMHandler, MetadataConstrainedLogitsProcessor, FSMState


def borrow(cls, *names):
    """A class whose methods are ``cls``'s own functions, and nothing else of it."""
    return type("Borrowed" + cls.__name__, (), {n: cls.__dict__[n] for n in names})


def stage_settings(V):
    temps, pens = (None, 0.7, 0.0), (1.0, 1.1, 1.3)
    if V <= 65:
        return [(m, T, p) for m in O.MODE_NAMES for T in temps for p in pens]
    if V == 1003:
        return [(m, T, p) for m in O.MODE_NAMES for T, p in ((None, 1.0), (0.7, 1.1), (0.0, 1.3), (0.7, 1.3))]
    return [(m, (None, 0.7, 0.0)[i % 3], (1.3, 1.0, 1.1)[i % 3]) for i, m in enumerate(O.MODE_NAMES)]


def main():
    H, P, FSM = import_reference()
    Proc = borrow(P, "__call__", "_apply_temperature_scaling", "update_state", "_input_contains_think_end_tag")
    out = {}

    # ------------------------------------------------------------------ (a) the stage
    Vs = (1, 31, 32, 33, 65, 1003, 2051)
    out["n_stage"] = np.int64(len(Vs))
    for c, V in enumerate(Vs):
        g = torch.Generator().manual_seed(SEED0 + c)
        cond = (torch.randn(3, V, generator=g) * 3).numpy()
        uncond = (torch.randn(3, V, generator=g) * 3).numpy()
        rng = np.random.default_rng(SEED0 + c)
        eos = V - 1 if V < 1000 else 950
        pad = max(0, V - 2)
        mask = np.where(rng.random(V) < 0.5, 0.0, -np.inf).astype(np.float32)
        mask[eos] = 0.0
        amask = np.where(mask == 0, -np.inf, 0.0).astype(np.float32)
        hist = rng.integers(0, V, size=(3, 9))
        hist[:, :2] = pad
        hist[:, 4] = hist[:, 3]
        if V == 65:     # signed zeros: every pairing, in the history (the penalty divides a zero) and out of it
            for i, (a, b) in enumerate(((-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0), (0.0, 0.0))):
                cond[:, 2 * i:2 * i + 2] = a
                uncond[:, 2 * i:2 * i + 2] = b
                hist[:, 5] = 0
                hist[:, 6] = 2
                hist[:, 7] = 4
                hist[:, 8] = 6
            mask[:8] = 0.0
        if V == 33:     # -inf - -inf: NaN from the combine on
            cond[:, 5] = -np.inf
            uncond[:, 5] = -np.inf
            cond[1, 6] = -np.inf
        sets = stage_settings(V)
        out[f"s{c}_cond"], out[f"s{c}_uncond"], out[f"s{c}_mask"], out[f"s{c}_amask"] = cond, uncond, mask, amask
        out[f"s{c}_eos"], out[f"s{c}_hist"] = np.int64(eos), hist.astype(np.int64)
        out[f"s{c}_mode"] = np.array([O.MODE_NAMES.index(m) for m, _T, _p in sets], dtype=np.int32)
        out[f"s{c}_T"] = np.array([np.nan if T is None else T for _m, T, _p in sets], dtype=np.float64)
        out[f"s{c}_pen"] = np.array([p for _m, _T, p in sets], dtype=np.float64)
        case = (cond, uncond, {"codes": mask, "audio": amask}, eos, hist, None)
        for s, (mode, T, pen) in enumerate(sets):
            p = Proc()
            p.enabled = mode != "disabled"
            p.debug = False
            p.state = {"disabled": FSM.THINK_TAG, "understand": FSM.COMPLETED, "completed": FSM.COMPLETED}.get(mode, FSM.CODES_GENERATION)
            p.generation_phase = "understand" if mode == "understand" else "codes"
            p.audio_code_mask = torch.from_numpy(amask.copy())[None, :]
            p.non_audio_code_mask = torch.from_numpy(mask.copy())[None, :]
            p.eos_token_id = eos
            p.target_codes = {"block": 10, "force": 10}.get(mode)
            p.codes_count = 10 if mode == "force" else 3
            p.codes_temperature = p.metadata_temperature = T
            ids = torch.from_numpy(hist.astype(np.int64))
            cl, ul = torch.from_numpy(cond.copy()), torch.from_numpy(uncond.copy())
            x = ul.float() + O.CFG_SCALE * (cl.float() - ul.float())     # llm_inference.py:2482
            x = p(ids, x)
            for lp in H._build_logits_processor(None, pen):
                x = lp(ids, x)
            got = x.numpy().astype(np.float32)
            assert O.same_bits(O.expected_for(case, (mode, T, pen, None)), got), (V, mode, T, pen)
            out[f"s{c}_out{s}"] = got
        print("stage", V, len(sets), "settings; NaNs", int(np.isnan(out[f"s{c}_out0"]).sum()))

    # ------------------------------------------------------------------ (b) the loop
    Handler = borrow(H, "_generate_with_cfg_custom", "_build_logits_processor", "_forward_pass", "_apply_top_k_filter",
                     "_apply_top_p_filter", "_sample_tokens", "_update_constrained_processor_state", "_check_eos_token")
    for name, B, target, pen, T, seed in L.loop_cases():
        ids, am = L.loop_prompt(B)
        mine = L.make_processor(target, T)
        p = Proc()
        for k, v in vars(mine).items():
            setattr(p, k, v.clone() if isinstance(v, torch.Tensor) else v)
        p.state = FSM.THINK_TAG
        h = Handler()
        h.llm, h.device, h.disable_tqdm = L.FakeModel(seed), "cpu", True
        h.llm_tokenizer = L.FakeTokenizer(L.EOS)
        got = h._generate_with_cfg_custom(ids, am, L.MAX_NEW, 0.0, L.CFG_SCALE, None, None, pen, L.PAD, None, p)
        steps = got.shape[1] - ids.shape[1]
        new = got[:B, ids.shape[1]:]
        assert torch.equal(got[:B, ids.shape[1]:], got[B:, ids.shape[1]:]) and bool((new[:, -1] == L.EOS).any()), (name, new)
        assert 2 <= steps < L.MAX_NEW, (name, steps)
        if target is not None:   # the quirk: the count advances by B per step, so ceil(target / B) code steps, then the forced EOS
            assert steps == -(-target // B) + 1 and bool((new[:, -1] == L.EOS).all()), (name, steps)
        model = L.FakeModel(seed)
        again = L.run_loop(lambda g, step: model(g if step == 0 else g[:, -1:], torch.ones(g.shape), None if step == 0 else 1).logits[:, 0],
                           L.torch_stage(L.CFG_SCALE, pen), lambda x: torch.argmax(x, dim=-1), ids, L.MAX_NEW, L.EOS, L.PAD, mine)
        assert torch.equal(again, got) and mine.state.name == p.state.name and mine.codes_count == p.codes_count, name
        out[f"l_{name}_ids"] = got.numpy().astype(np.int64)
        out[f"l_{name}_state"] = np.array(p.state.name)
        out[f"l_{name}_count"] = np.int64(p.codes_count)
        print("loop", name, "steps", steps, "state", p.state.name, "count", p.codes_count, new.tolist())
    dst = os.path.join(HERE, "g23_lm_logits.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
