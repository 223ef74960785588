"""CPU: the 5 Hz LM's non-CFG path with no GPU - the bf16 stage's numpy oracle and the loop restatement against what the reference
recorded (G26), the control flow of ``generate_constrained`` / ``generate_codes_batch_nocfg`` (the production functions) on stand-ins
(tests/_lm_nocfg_stubs.py), the pure ``nocfg_batch_request``, the new export's signature and refusals (all made before any HIP call)
and the mixin's pass-through."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import _lm_logits_oracle as O
import _lm_loop_ref as R
import _lm_nocfg_oracle as N
import _lm_nocfg_ref as NR
import _lm_nocfg_stubs as St

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
TEMP, TOP_P = 0.85, 0.9


# ------------------------------------------------------------------ G26 (a): the stage
def test_g26_oracle_equals_reference_bit_for_bit():
    assert os.path.getsize(N.G26) <= 1 << 20
    cases = N.load_g26_stage()
    assert [c[0].shape for c in cases] == [(3, V) for V in N.STAGE_V]
    n = 0
    for case in cases:
        assert N.is_bf16(case[0])                                  # the logits are a bf16 model's
        seen_modes, seen_T, seen_pen = set(), set(), set()
        for setting in case[4]:
            mode, T, pen, want = setting
            assert N.is_bf16(want) and O.same_bits(N.expected_for(case, setting), want), (case[0].shape, mode, T, pen)
            seen_modes.add(mode), seen_T.add(T), seen_pen.add(pen)
            n += 1
        assert seen_modes == set(O.MODES) and seen_T == {None, 0.7, 0.6, 0.0} and seen_pen == {1.0, 1.1, 1.3}
    assert n == 5 * 72 + 30 + 6


def test_g26_holds_the_edge_inputs_and_the_fp32_stage_would_not_do():
    cases = N.load_g26_stage()
    cond, _m, _e, hist, _s = cases[4]                            # V = 65: signed zeros, in and out of the history
    assert np.signbit(cond[0, 0]) and cond[0, 0] == 0 and not np.signbit(cond[0, 4]) and {0, 2, 4, 6} <= set(hist[0].tolist())
    assert cases[3][0][0, 5] == NEG                              # V = 33: a -inf logit
    ties = differ = 0
    for cond, masks, eos, hist, sets in cases[1:6]:              # quotients by 0.6 that are ties between two bf16 neighbours
        for mode, T, pen, want in sets:
            if T == 0.6 and mode in ("none", "block", "disabled", "completed"):
                pre = N.expected_for((cond, masks, eos, hist, None), (mode, None, 1.0, None))
                k = int(N.halfway_mask(pre, 0.6).sum())
                assert k >= 3, (cond.shape, mode)
                ties += k
            which, eos_mode = O.MODES[mode]
            fp32 = O.shape(cond, None, 1.0, masks[which] if which else None, eos, eos_mode, T, pen, O.seen_bitmap(hist, cond.shape[1]))
            differ += int(not O.same_bits(fp32, want))
    assert ties > 1000 and differ > 100                          # (the fp32 stage gives other bits wherever something is divided)


def test_rne_rules():
    f = np.float32
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, np.inf, -np.inf, 0.0, -0.0, np.nan, 3.4e38, 1e-40, 4.6e-41], dtype=f)
    r = N.rne(x)
    # 1 + 2^-8 is a tie: down to the even 1.0; 1 + 3 * 2^-8 is a tie: up to the even 1 + 2^-6
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == f(1.015625) and r[3] == -1.0
    assert r[4] == np.inf and r[5] == -np.inf and r[6] == 0 and not np.signbit(r[6]) and r[7] == 0 and np.signbit(r[7]) and np.isnan(r[8])
    assert r[9] == np.inf                                        # past bf16's largest finite value
    assert N.is_bf16(r) and r[10] > 0 and r[11] > 0              # subnormals round like any value
    t = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert O.same_bits(r, t)                                     # torch's own cast
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(1 << 16, generator=g) * 5).numpy()
    assert O.same_bits(N.rne(y), torch.from_numpy(y).to(torch.bfloat16).float().numpy())
    c = np.array([[1.00390625, -2.0, 0.5, -0.0]], dtype=f)
    assert N.shape(c)[0].tolist() == [1.0, -2.0, 0.5, -0.0] and np.signbit(N.shape(c)[0, 3])
    assert not np.signbit(N.shape(c, mask=np.zeros(4, dtype=f))[0, 3])
    assert N.shape(c, eos_id=1, eos_mode=O.EOS_FORCE)[0].tolist() == [NEG, -2.0, NEG, NEG]
    assert N.shape(c, temperature=0.6)[0, 0] == N.rne(np.array([f(1.0) / f(0.6)], dtype=f))[0]
    assert N.shape(c, penalty=1.3, seen=O.seen_bitmap([[0, 1]], 4))[0, 1] == N.rne(np.array([f(-2.0) * f(1.3)], dtype=f))[0]
    assert O.same_bits(N.shape_as(c, "fp32", temperature=0.6), O.shape(c, temperature=0.6))


# ------------------------------------------------------------------ G26 (b): the loop
@pytest.mark.parametrize("case", NR.loop_cases(), ids=lambda c: c[0])
def test_loop_restatement_reproduces_the_reference(case):
    name, dt, B, phase, pen, T, _seed0 = case
    want_ids, want_state, want_count, seed = NR.load_g26_loop()[name]
    ids, _am = NR.loop_prompt(B)
    proc = NR.make_processor(phase, T)
    got = NR.run_loop(NR.forward_of(NR.FakeModel(seed, NR.DTYPES[dt])), NR.torch_stage(NR.DTYPES[dt], pen), NR.unique_argmax, ids, NR.MAX_NEW,
                      R.EOS, R.PAD, proc)
    assert np.array_equal(got.numpy(), want_ids) and (want_ids[:, -1] == R.EOS).any()
    if proc is None:
        assert (want_state, want_count) == ("", -1)
    else:
        assert proc.state.name == want_state and proc.codes_count == want_count
        assert want_state == {"understand": "COMPLETED", "disabled": "THINK_TAG"}.get(phase, "CODES_GENERATION")


def _steps_expected(phase, steps, B):
    """(native steps, sync-free steps, token reads) of a loop of ``steps`` steps without a streamer."""
    if phase == "target":        # step 0 is the reference's processor (THINK_TAG -> CODES_GENERATION), the last step forces EOS
        return steps - 1, steps - 2, 2
    if phase == "free":
        return steps - 1, 0, steps
    return steps, 0, steps       # COMPLETED, a disabled processor, no processor: native from step 0, every token read


def _lm_calls(log):
    return [c for c in log if c in ("prefill", "decode_tokens", "fan_out", "bad_tokens")]


@pytest.mark.parametrize("case", NR.loop_cases(), ids=lambda c: c[0])
def test_native_loop_reproduces_the_recorded_reference_loops(monkeypatch, case):
    from ace355.lmlogits import generate_constrained
    name, dt, B, phase, pen, T, _seed0 = case
    dtype = NR.DTYPES[dt]
    log, shapes = St.install(monkeypatch, St.unique_argmax_pick)
    want_ids, want_state, want_count, seed = NR.load_g26_loop()[name]
    ids, am = NR.loop_prompt(B)
    proc, h, lm = NR.make_processor(phase, T), St.StubHandler(), St.StubLm(seed, log, dtype)
    got = generate_constrained(h, lm, ids, am, NR.MAX_NEW, 0.0, None, None, pen, R.PAD, None, proc)
    assert got.dtype == ids.dtype and np.array_equal(got.numpy(), want_ids)
    if proc is not None:
        assert proc.state.name == want_state and proc.codes_count == want_count
    stats = h._lm_loop_stats
    steps = want_ids.shape[1] - ids.shape[1]
    native_steps, sync_free, reads = _steps_expected(phase, steps, B)
    assert set(stats) == {"steps", "native_steps", "sync_free_steps", "token_reads", "cfg"} and stats["cfg"] is False
    assert (stats["steps"], stats["native_steps"], stats["sync_free_steps"], stats["token_reads"]) == (steps, native_steps, sync_free, reads)
    assert shapes == [(dtype, B, False)] * native_steps           # the stage in the model's dtype, B rows, no unconditional ones
    assert _lm_calls(log) == ["bad_tokens", "prefill"] + ["decode_tokens"] * (steps - 1) + ["bad_tokens"]
    marks = ["mark"] if pen != 1.0 else []
    body = [c for c in log if c not in ("prefill", "decode_tokens", "bad_tokens")]
    first = ["select"] if native_steps < steps else ["shape", "pick"]
    assert body == marks + first + marks + (["shape", "pick"] + marks) * (steps - 1)
    assert lm.fed == [want_ids[:, ids.shape[1] + t].tolist() for t in range(steps - 1)]


def test_native_loop_with_a_streamer_reads_every_step(monkeypatch):
    from ace355.lmlogits import generate_constrained
    name = "bf16_B2_target_p1.0"
    log, _shapes = St.install(monkeypatch, St.unique_argmax_pick)
    want_ids, _state, want_count, seed = NR.load_g26_loop()[name]
    ids, am = NR.loop_prompt(2)
    proc, h, s = NR.make_processor("target", None), St.StubHandler(), St.Streamer()
    got = generate_constrained(h, St.StubLm(seed, log, torch.bfloat16), ids, am, NR.MAX_NEW, 0.0, None, None, 1.0, R.PAD, s, proc)
    assert np.array_equal(got.numpy(), want_ids) and proc.codes_count == want_count
    stats = h._lm_loop_stats
    assert stats["steps"] == 4 and stats["sync_free_steps"] == 0 and stats["token_reads"] == 4
    assert s.ended == 1 and len(s.put_calls) == 4
    assert all(p.shape == (2, 1) and torch.equal(p[:, 0], got[:, 6 + t]) for t, p in enumerate(s.put_calls))


def test_native_loop_stops_on_the_pad_id_and_raises_for_a_bad_draw(monkeypatch):
    from ace355.lmlogits import generate_constrained
    log, _shapes = St.install(monkeypatch, St.argmax_pick)
    ids, am = NR.loop_prompt(2)
    h = St.StubHandler()
    lm = St.StubLm(5, log, torch.bfloat16, boost=(1, 1, R.PAD))    # step 1, row 1 draws the pad id: _check_eos_token's second rule
    got = generate_constrained(h, lm, ids, am, NR.MAX_NEW, 0.0, None, None, 1.0, R.PAD, None, None)
    assert got.shape == (2, 8) and got[1, 7] == R.PAD and got[0, 7] != R.PAD
    log2, _shapes = St.install(monkeypatch, St.argmax_pick)
    lm = St.StubLm(5, log2, torch.bfloat16, nan_step=2)
    with pytest.raises(RuntimeError, match=r"no valid token .* advanced 3 steps"):
        generate_constrained(h, lm, ids, am, NR.MAX_NEW, 0.0, None, None, 1.0, R.PAD, None, None)
    assert h._lm_loop_stats["steps"] == 3 and len(lm.fed) == 2
    lm = St.StubLm(5, log2, torch.float16)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        generate_constrained(h, lm, ids, am, NR.MAX_NEW, 0.0, None, None, 1.0, R.PAD, None, None)
    assert lm.step == 0                                          # refused before the prefill


def test_the_cfg_modes_still_call_the_stage_with_the_old_signature(monkeypatch):
    """tests/_lm_loop_stubs.py replaces ``shape_logits`` with a function that takes no ``dtype``: the CFG loop must not pass one."""
    import _lm_loop_stubs as Old
    from ace355.lmlogits import generate_with_cfg
    log = Old.install(monkeypatch, Old.argmax_pick)
    name, B, target, pen, T, seed = R.loop_cases()[5]
    ids, am = R.loop_prompt(B)
    h = Old.StubHandler()
    got = generate_with_cfg(h, Old.StubLm(seed, log), ids, am, R.MAX_NEW, 0.0, R.CFG_SCALE, None, None, pen, R.PAD, None, R.make_processor(target, T))
    assert np.array_equal(got.numpy(), R.load_g23_loop()[name][0]) and "cfg" not in h._lm_loop_stats


# ------------------------------------------------------------------ B songs in one loop
def _sequential(monkeypatch, seed, dtype, target, pen, T, max_new):
    from ace355.lmlogits import generate_constrained
    log, _shapes = St.install(monkeypatch, St.oracle_pick)
    ids, am = NR.loop_prompt(1)
    proc, h = R.make_processor(target, T), St.StubHandler()
    torch.manual_seed(seed)
    out = generate_constrained(h, St.StubLm(7, log, dtype, St.song_logits), ids, am, max_new, TEMP, None, TOP_P, pen, R.PAD, None, proc)
    return out[0], proc


@pytest.mark.parametrize("B,dtype,target,pen,T", [(2, torch.bfloat16, 6, 1.0, None), (3, torch.bfloat16, 10, 2.0, 0.5),
                                                  (16, torch.bfloat16, 6, 1.3, 0.85), (3, torch.float32, 6, 1.3, 0.85)],
                         ids=["B2", "B3_penalty2_T0.5", "B16", "B3_fp32"])
def test_batched_loop_rows_equal_the_sequential_loop_per_seed(monkeypatch, B, dtype, target, pen, T):
    from ace355.lmlogits import generate_codes_batch_nocfg
    seeds = [3, 11, 3, 29, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987][:B]
    seq = [_sequential(monkeypatch, s, dtype, target, pen, T, 14) for s in seeds]
    want = torch.stack([row for row, _p in seq])
    log, shapes = St.install(monkeypatch, St.oracle_pick)
    ids, am = NR.loop_prompt(1)
    proc, h, lm = R.make_processor(target, T), St.StubHandler(), St.StubLm(7, log, dtype, St.song_logits)
    torch.manual_seed(1234)
    rng = torch.get_rng_state()
    got = generate_codes_batch_nocfg(h, lm, ids, am, seeds, 14, TEMP, None, TOP_P, pen, R.PAD, proc)
    assert torch.equal(torch.get_rng_state(), rng)                # the global generator is not touched
    assert got.dtype == torch.int64 and torch.equal(got, want)
    if B > 2:
        assert torch.equal(got[0], got[2]) and len({tuple(r.tolist()) for r in got}) == B - 1
    steps = target + 1
    assert got.shape == (B, 6 + steps) and (got[:, -1] == R.EOS).all()
    assert proc.codes_count == seq[-1][1].codes_count == steps and proc.state == seq[-1][1].state == R.FSMState.CODES_GENERATION
    stats = h._lm_loop_stats
    assert stats["batch"] == B and stats["prefill_rows"] == 1 and stats["steps"] == steps and stats["cfg"] is False
    assert stats["native_steps"] == steps - 1 and stats["sync_free_steps"] == steps - 2 and stats["token_reads"] == 2
    assert shapes == [(dtype, B, False)] * (steps - 1)
    assert lm.fan_outs == [[0] * B]                               # once, after step 0's tokens are selected and before the first decode
    assert _lm_calls(log) == ["bad_tokens", "prefill", "fan_out"] + ["decode_tokens"] * (steps - 1) + ["bad_tokens"]
    assert log.index("pick") < log.index("fan_out") < log.index("decode_tokens") and "select" not in log
    assert lm.fed == [got[:, 6 + t].tolist() for t in range(steps - 1)]


def test_batched_loop_refusals(monkeypatch):
    from ace355.lmlogits import generate_codes_batch_nocfg
    log, _shapes = St.install(monkeypatch, St.oracle_pick)
    ids, am = NR.loop_prompt(1)
    h = St.StubHandler()

    def run(proc, seeds=(1, 2), ids=ids, am=am, dtype=torch.bfloat16, max_seqs=16, eos=R.EOS, boost=None):
        return generate_codes_batch_nocfg(St.StubHandler(eos) if eos != R.EOS else h, St.StubLm(7, log, dtype, St.song_logits, boost=boost,
                                          max_seqs=max_seqs), ids, am, list(seeds), 8, TEMP, None, TOP_P, 1.0, R.PAD, proc)
    for change in ({"target_codes": None}, {"enabled": False}, {"eos_token_id": None}, None):
        proc = None
        if change is not None:
            proc = R.make_processor(6, None)
            for k, v in change.items():
                setattr(proc, k, v)
        with pytest.raises(RuntimeError, match="needs an enabled constrained processor with target_codes and eos_token_id"):
            run(proc)
    with pytest.raises(ValueError, match="17 songs need 17 sequences, the native LM holds 16"):
        run(R.make_processor(6, None), seeds=range(17))
    with pytest.raises(ValueError, match="3 songs need 3 sequences, the native LM holds 2"):
        run(R.make_processor(6, None), seeds=range(3), max_seqs=2)
    with pytest.raises(ValueError, match="0 songs need 0 sequences"):
        run(R.make_processor(6, None), seeds=())
    with pytest.raises(ValueError, match=r"takes the \[1, P\] ids"):
        run(R.make_processor(6, None), ids=NR.loop_prompt(2)[0], am=None)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        run(R.make_processor(6, None), dtype=torch.float16)
    assert log == []
    # the tokenizer's EOS is an id the codes mask allows (the processor blocks another): step 2's logits push it on song 1 only
    with pytest.raises(RuntimeError, match=r"songs \[1\] of 2 stopped at step 2 and the others did not"):
        run(R.make_processor(40, None), eos=500, boost=(2, 1, 500))


# ------------------------------------------------------------------ the seam's conditions
GOOD = dict(formatted_prompts=["p", "p", "p"], cfg_scale=1.0, generation_phase="codes", use_constrained_decoding=True,
            target_duration=30.0, seeds=[1, 2, 3])


def test_nocfg_batch_request_accepts_the_reference_batch_call_without_cfg():
    from ace355.lmlogits import batch_request, nocfg_batch_request
    assert nocfg_batch_request(**GOOD) == (True, None)
    assert nocfg_batch_request(**{**GOOD, "seeds": (4, 5, 6, 7), "cfg_scale": 0.5}) == (True, None)
    assert nocfg_batch_request(**{**GOOD, "cfg_scale": float("nan")}) == (True, None)      # `not cfg_scale > 1.0`, as the reference branches
    assert batch_request(**GOOD)[0] is False                     # the CFG batch refuses what this one takes ...
    assert batch_request(**{**GOOD, "cfg_scale": 2.0}) == (True, None)                     # ... and takes what this one refuses


@pytest.mark.parametrize("change,text", [
    ({"formatted_prompts": "p"}, "not a list"), ({"formatted_prompts": ["p"]}, "not a list"),
    ({"formatted_prompts": ["p", "p", "q"]}, "differ"),
    ({"cfg_scale": 1.5}, "cfg_scale 1.5 runs a CFG pair"),
    ({"generation_phase": "understand"}, "phase"),
    ({"use_constrained_decoding": False}, "constrained decoding"),
    ({"target_duration": None}, "target duration"), ({"target_duration": 0}, "target duration"),
    ({"seeds": None}, "seeds"), ({"seeds": [1, 2]}, "seeds"), ({"seeds": [1, None, 3]}, "seeds"), ({"seeds": [1, True, 3]}, "seeds"),
    ({"loop_refusal": "17 sequences exceed the native handle"}, "exceed the native handle")])
def test_nocfg_batch_request_names_the_reason_for_each_refusal(change, text):
    from ace355.lmlogits import nocfg_batch_request
    ok, why = nocfg_batch_request(**{**GOOD, **change})
    assert ok is False and text in why


# ------------------------------------------------------------------ the C ABI
def test_shape_as_in_header_library_and_signatures():
    from ace355 import native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ace355.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ace355_lm_shape_as\s*\([^)]*const\s+ace355_lm_shape_params\s*\*\s*\w+\s*,\s*int\s+dtype\s*,\s*void\s*\*\s*stream\s*\)", src)
    for name, value in (("ACE355_DTYPE_F32", native.DTYPE_F32), ("ACE355_DTYPE_BF16", native.DTYPE_BF16)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1)) == value
    assert hasattr(native.lib(), "ace355_lm_shape_as")
    restype, argtypes = native.SIGNATURES["ace355_lm_shape_as"]
    old = native.SIGNATURES["ace355_lm_shape"][1]
    assert restype is ctypes.c_int and argtypes == old[:-1] + [ctypes.c_int, ctypes.c_void_p]
    assert ctypes.sizeof(native.LmShapeParamsC) == 40             # the params struct did not grow: the dtype travels beside it


SHAPE_AS_REFUSALS = {"dtype_unknown": "dtype must", "dtype_negative": "dtype must", "uncond_bf16": "fp32 only", "B_zero": "B must",
                     "B_large": "B must", "V_zero": "V must", "V_large": "V must", "cond_stride": "stride", "out_stride": "stride",
                     "uncond_stride_f32": "stride", "null_cond": "null", "null_out": "null", "null_params": "null", "eos_low": "eos_id",
                     "eos_high": "eos_id", "eos_mode": "eos_mode", "penalty_zero": "penalty", "penalty_negative": "penalty",
                     "penalty_inf": "penalty", "penalty_nan": "penalty", "null_seen": "seen", "temperature_zero": "temperature",
                     "temperature_nan": "temperature", "cfg_nan_f32": "cfg_scale"}


@pytest.mark.parametrize("case", list(SHAPE_AS_REFUSALS))
def test_shape_as_refusals_need_no_gpu(case):
    """Each defect alone is refused with ACE355_ERR_INVALID and a message before any HIP call: the pointers here are not memory."""
    from ace355 import native
    lib = native.lib()
    V = 100
    a = dict(cond=4096, cs=V, uncond=None, us=0, out=4096, os=V, B=2, V=V, dtype=native.DTYPE_BF16)
    p = dict(cfg_scale=2.0, eos_id=5, eos_mode=1, has_temperature=1, temperature=0.85, penalty=1.1, mask=4096, seen=4096)
    if case == "dtype_unknown":
        a["dtype"] = 2
    elif case == "dtype_negative":
        a["dtype"] = -1
    elif case == "uncond_bf16":
        a.update(uncond=8192, us=V)
    elif case == "B_zero":
        a["B"] = 0
    elif case == "B_large":
        a["B"] = native.LM_MAX_SEQS + 1
    elif case == "V_zero":
        a["V"] = 0
    elif case == "V_large":
        a["V"] = a["cs"] = a["os"] = native.LM_PICK_MAX_V + 1
    elif case in ("cond_stride", "out_stride"):
        a[{"cond_stride": "cs", "out_stride": "os"}[case]] = V - 1
    elif case == "uncond_stride_f32":
        a.update(uncond=8192, us=V - 1, dtype=native.DTYPE_F32)
    elif case == "null_cond":
        a["cond"] = None
    elif case == "null_out":
        a["out"] = None
    elif case == "eos_low":
        p["eos_id"] = -1
    elif case == "eos_high":
        p["eos_id"] = V
    elif case == "eos_mode":
        p["eos_mode"] = 3
    elif case.startswith("penalty_"):
        p["penalty"] = {"zero": 0.0, "negative": -1.5, "inf": float("inf"), "nan": float("nan")}[case[8:]]
    elif case == "null_seen":
        p["seen"] = None
    elif case.startswith("temperature_"):
        p["temperature"] = {"zero": 0.0, "nan": float("nan")}[case[12:]]
    elif case == "cfg_nan_f32":
        a.update(uncond=8192, us=V, dtype=native.DTYPE_F32)
        p["cfg_scale"] = float("nan")
    params = native.LmShapeParamsC(**p)
    lib.ace355_lm_pick_plan(0, None, None)   # leaves another message behind
    rc = lib.ace355_lm_shape_as(a["cond"], a["cs"], a["uncond"], a["us"], a["out"], a["os"], a["B"], a["V"],
                                None if case == "null_params" else ctypes.byref(params), a["dtype"], None)
    assert rc == 1 and "lm_shape_as:" in native.last_error() and SHAPE_AS_REFUSALS[case] in native.last_error(), native.last_error()


def test_shape_logits_refuses_other_dtypes_before_it_looks_at_the_tensors():
    from ace355.lmlogits import shape_logits
    x = torch.zeros(2, 10)
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="torch.float32 or torch.bfloat16"):
            shape_logits(x, dtype=bad)
    with pytest.raises(ValueError, match="takes no uncond"):
        shape_logits(x, x, dtype=torch.bfloat16)


# ------------------------------------------------------------------ the mixin, where it must not change anything
class _Base:
    def __init__(self):
        self.calls, self.runs = [], []

    def _generate_with_constrained_decoding(self, *args):
        self.calls.append(args)
        return "reference"

    def _run_pt(self, formatted_prompts, *a, **k):
        self.runs.append((formatted_prompts, a, k))
        return "host"


def _handler(flag):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _Base):
        pass

    h = Handler()
    if flag is not None:
        h.use_native_lm_nocfg = flag
    return h


@pytest.mark.parametrize("flag", [None, False, True])
def test_override_passes_through_when_off_or_when_the_request_does_not_fit(flag, monkeypatch, caplog):
    """Flag off (the default without ACE355_LM_NOCFG=1), or on with ids on the CPU: the host's loop gets the very arguments, and the
    native loop is never asked."""
    from ace355 import backend, lmlogits
    if flag is None:
        assert backend.NativeLmMixin.use_native_lm_nocfg is (os.environ.get("ACE355_LM_NOCFG", "") == "1")
        flag = False

    def boom(*a, **k):
        raise AssertionError("the native loop must not be called")
    monkeypatch.setattr(lmlogits, "generate_constrained", boom)
    monkeypatch.setattr(lmlogits, "generate_codes_batch_nocfg", boom)
    caplog.set_level("INFO", logger="ace355")
    h = _handler(flag)
    h.llm = types.SimpleNamespace()
    ids, am = NR.loop_prompt(2)
    proc, streamer = object(), object()
    for _ in range(2):
        assert h._generate_with_constrained_decoding(ids, am, 12, 0.85, None, 0.9, 1.0, R.PAD, streamer, proc) == "reference"
    assert len(h.calls) == 2
    got = h.calls[0]
    assert got[0] is ids and got[1] is am and got[2:8] == (12, 0.85, None, 0.9, 1.0, R.PAD) and got[8] is streamer and got[9] is proc
    assert h._lm_loop_stats is None
    said = [r.getMessage() for r in caplog.records if "[native-lm-nocfg]" in r.getMessage()]
    assert (len(said) == 1 and "CUDA device" in said[0] and "[B, P]" in said[0]) if flag else not said   # asked for: said once
    # _run_pt: the host's method gets the call with its arguments; with the flag on a batch that misses a condition says why once
    caplog.clear()
    args = (0.85, 1.0, "NO USER INPUT", None, 0.9, 1.0)
    for _ in range(2):
        assert h._run_pt(["p", "q"], *args, generation_phase="codes", target_duration=30.0, seeds=[1, 2]) == "host"
    assert h._run_pt("p", *args, generation_phase="understand") == "host"                   # a single prompt: nothing to say
    assert h._run_pt(["p", "p"], 0.85, 2.0, *args[2:], generation_phase="codes", target_duration=30.0, seeds=[1, 2]) == "host"   # CFG: not this flag's
    assert len(h.runs) == 4 and h.runs[0][0] == ["p", "q"] and h.runs[0][1] == args and h.runs[0][2]["seeds"] == [1, 2]
    said = [r.getMessage() for r in caplog.records if "[native-lm-nocfg]" in r.getMessage()]
    assert (len(said) == 1 and "differ" in said[0] and "item by item" in said[0]) if flag else not said
    assert not [r for r in caplog.records if "[native-lm-batch]" in r.getMessage()]          # (that flag is off: as before)


def test_override_keeps_the_reference_signature_and_the_loop_check_its_answers():
    import inspect
    from ace355.backend import NativeLmMixin
    names = list(inspect.signature(NativeLmMixin._generate_with_constrained_decoding).parameters)
    assert names == ["self", "input_ids", "attention_mask", "max_new_tokens", "temperature", "top_k", "top_p", "repetition_penalty",
                     "pad_token_id", "streamer", "constrained_processor"]
    h = _handler(True)
    ids, am = NR.loop_prompt(1)
    assert h._lm_loop_accepts(ids, am, 4) == (None, "the input ids are not a [2B, P] tensor on a CUDA device")   # as for its callers so far
    assert h._lm_loop_accepts(ids, am, 4, pairs=False) == (None, "the input ids are not a [B, P] tensor on a CUDA device")
