#!/usr/bin/env python
"""Generate g26_lm_nocfg.npz: what the reference's own logits stage and non-CFG loop compute on bf16 logits (build container only, like
make_g23_lm_logits.py, whose way of importing the reference this follows: the classes on the CPU, a ``loguru`` stub, methods borrowed
onto plain namespaces).  Arrays only.

(a) Stage cases, V in {1, 31, 32, 33, 65, 1003, 2051}, B = 3: seeded ``randn * 3`` logits cast to bf16 (stored as the fp32 values the
bf16 numbers have), the masks and histories of G23's cases.  Per setting (processor branch; temperature none / 0.7 / 0.6 / 0; penalty
1 / 1.1 / 1.3) the file holds ``MetadataConstrainedLogitsProcessor.__call__`` followed by the list ``_build_logits_processor`` returns,
on the bf16 tensor, as fp32.  The small V take all 72 settings, V = 1003 takes 30, V = 2051 one per branch.  Planted: signed zeros
(V = 65), a -inf logit (V = 33), and from V = 31 on bf16 values whose fp32 quotient by T lies exactly half-way between two bf16
neighbours, in and out of the history.  Such values exist for T = 0.6 only: the script searches all 65536 bf16 bit patterns per T,
asserts that 0.7 and 1e-6 have none at all (so nothing can be planted for them) and that every T = 0.6 setting that keeps the
planted ids finite divides at least one of them.  The script asserts that tests/_lm_nocfg_oracle.py gives the same bits.

(b) Loop cases: the reference's real ``_generate_with_constrained_decoding`` on tests/_lm_nocfg_ref.py's CPU fake model (its logits
cast to the case's dtype), greedy; dtype bf16 / fp32, B = 1 / 2; phases "understand" (``COMPLETED`` with an ``audio_code_mask``, EOS
reachable), codes with target 6, codes without a target, a disabled processor, no processor; penalty / temperature off and 1.3 /
0.85.  Per case: the ids, the processor's final state and count, and the model seed.  The maximum must be unique at every greedy
step (bf16 makes ties likely, and a tie would leave the token to argmax's tie-break): a seed that violates this is replaced by the
next one (+1000).  The script asserts that tests/_lm_nocfg_ref.py reproduces each.

Everything is random logits; nothing here says anything about a trained LM's token stream.

Usage:  python tests/golden/make_g26_lm_nocfg.py
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
import _lm_nocfg_oracle as N  # noqa: E402
import _lm_nocfg_ref as NR  # noqa: E402

REF = "/root/reference"
SEED0 = 2600
PLANT = (10, 11, 12, 13)   # ids that carry the half-way values (V >= 31)


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


def halfway_values():
    """T -> every finite bf16 value whose fp32 quotient by T is a tie between two bf16 neighbours (all 65536 patterns searched)."""
    x = (np.arange(65536, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    x = x[np.isfinite(x)]
    return {T: x[N.halfway_mask(x, T)] for T in (0.7, 0.6, O.MIN_T)}


def main():
    H, P, FSM = import_reference()
    Proc = borrow(P, "__call__", "_apply_temperature_scaling", "update_state", "_input_contains_think_end_tag")
    out = {}

    # ------------------------------------------------------------------ (a) the stage
    half = halfway_values()
    assert len(half[0.7]) == 0 and len(half[O.MIN_T]) == 0, "a T thought to have no half-way quotient has one: plant it"
    h06 = half[0.6]
    h06 = h06[(np.abs(h06) > 0.5) & (np.abs(h06) < 12)]
    assert len(h06) >= 8
    plant = np.array([h06[h06 > 0][0], h06[h06 < 0][0], h06[h06 > 0][-1], h06[h06 < 0][-1]], dtype=np.float32)
    print("half-way at T = 0.6:", len(half[0.6]), "bf16 values; planted", plant.tolist())
    out["n_stage"] = np.int64(len(N.STAGE_V))
    for c, V in enumerate(N.STAGE_V):
        g = torch.Generator().manual_seed(SEED0 + c)
        cond = (torch.randn(3, V, generator=g) * 3).to(torch.bfloat16).float().numpy()
        rng = np.random.default_rng(SEED0 + c)
        eos = V - 1 if V < 1000 else 950
        pad = max(0, V - 2)
        mask = np.where(rng.random(V) < 0.5, 0.0, -np.inf).astype(np.float32)
        mask[eos] = 0.0
        hist = rng.integers(0, V, size=(3, 9))
        hist[:, :2] = pad
        hist[:, 4] = hist[:, 3]
        if V == 65:     # signed zeros, in the history (the penalty divides a zero) and out of it
            cond[:, 0:4] = -0.0
            cond[:, 4:8] = 0.0
            hist[:, 5], hist[:, 6], hist[:, 7], hist[:, 8] = 0, 2, 4, 6
            mask[:8] = 0.0
        if V == 33:     # a -inf logit
            cond[:, 5] = -np.inf
        if V >= 31:     # quotients by 0.6 that are ties; the first two also meet the penalty
            cond[:, list(PLANT)] = plant
            mask[list(PLANT)] = 0.0
            if V != 65:
                hist[:, 5], hist[:, 6] = PLANT[0], PLANT[1]
        amask = np.where(mask == 0, -np.inf, 0.0).astype(np.float32)
        assert N.is_bf16(cond)
        sets = N.stage_settings(V)
        out[f"s{c}_cond"], out[f"s{c}_mask"], out[f"s{c}_amask"] = cond, mask, amask
        out[f"s{c}_eos"], out[f"s{c}_hist"] = np.int64(eos), hist.astype(np.int64)
        out[f"s{c}_mode"] = np.array([O.MODE_NAMES.index(m) for m, _T, _p in sets], dtype=np.int32)
        out[f"s{c}_T"] = np.array([np.nan if T is None else T for _m, T, _p in sets], dtype=np.float64)
        out[f"s{c}_pen"] = np.array([p for _m, _T, p in sets], dtype=np.float64)
        case = (cond, {"codes": mask, "audio": amask}, eos, hist, None)
        ties = 0
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
            x = torch.from_numpy(cond.copy()).to(torch.bfloat16)     # outputs.logits[:, -1, :] of a bf16 model
            x = p(ids, x)
            for lp in H._build_logits_processor(None, pen):
                x = lp(ids, x)
            assert x.dtype == torch.bfloat16
            got = x.float().numpy()
            assert O.same_bits(N.expected_for(case, (mode, T, pen, None)), got), (V, mode, T, pen)
            if T == 0.6 and V >= 31 and mode in ("none", "block", "disabled", "completed"):   # ("understand" / force: the ids are -inf)
                n = int(N.halfway_mask(N.expected_for(case, (mode, None, 1.0, None)), 0.6).sum())
                assert n >= 3, (V, mode, n)
                ties += n
            out[f"s{c}_out{s}"] = got
        print("stage", V, len(sets), "settings; half-way quotients divided:", ties)

    # ------------------------------------------------------------------ (b) the loop
    Handler = borrow(H, "_generate_with_constrained_decoding", "_build_logits_processor", "_forward_pass", "_apply_top_k_filter",
                     "_apply_top_p_filter", "_sample_tokens", "_update_constrained_processor_state", "_check_eos_token")
    for name, dt, B, phase, pen, T, seed0 in NR.loop_cases():
        dtype = NR.DTYPES[dt]
        ids, am = NR.loop_prompt(B)
        for seed in range(seed0, seed0 + 20000, 1000):
            mine = NR.make_processor(phase, T)
            try:
                again = NR.run_loop(NR.forward_of(NR.FakeModel(seed, dtype)), NR.torch_stage(dtype, pen), NR.unique_argmax, ids, NR.MAX_NEW,
                                    L.EOS, L.PAD, mine)
            except AssertionError:
                continue
            break
        else:
            raise AssertionError(f"{name}: no seed without a tied greedy step")
        p = None
        if mine is not None:
            fresh = NR.make_processor(phase, T)
            p = Proc()
            for k, v in vars(fresh).items():
                setattr(p, k, v.clone() if isinstance(v, torch.Tensor) else v)
            p.state = FSM[fresh.state.name]
        h = Handler()
        h.llm, h.device, h.disable_tqdm = NR.FakeModel(seed, dtype), "cpu", True
        h.llm_tokenizer = L.FakeTokenizer(L.EOS)
        got = h._generate_with_constrained_decoding(ids, am, NR.MAX_NEW, 0.0, None, None, pen, L.PAD, None, p)
        steps = got.shape[1] - ids.shape[1]
        new = got[:, ids.shape[1]:]
        assert 2 <= steps < NR.MAX_NEW and bool((new[:, -1] == L.EOS).any()), (name, new)
        if phase == "target":   # the count advances by B per step, so ceil(target / B) code steps, then the forced EOS
            assert steps == -(-6 // B) + 1 and bool((new[:, -1] == L.EOS).all()), (name, steps)
        if phase == "understand":
            assert not bool(((new >= 300) & (new < 900)).any()), (name, new)
        assert torch.equal(again, got), name
        if p is not None:
            assert mine.state.name == p.state.name and mine.codes_count == p.codes_count, name
        out[f"l_{name}_ids"] = got.numpy().astype(np.int64)
        out[f"l_{name}_state"] = np.array(p.state.name if p is not None else "")
        out[f"l_{name}_count"] = np.int64(p.codes_count if p is not None else -1)
        out[f"l_{name}_seed"] = np.int64(seed)
        print("loop", name, "seed", seed, "steps", steps, "state", p.state.name if p else None, "count", p.codes_count if p else None, new.tolist())
    dst = os.path.join(HERE, "g26_lm_nocfg.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
