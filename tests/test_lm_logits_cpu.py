"""CPU: the LM logits stage's fixture against its numpy restatement, the recorded reference loops against the loop restatement, the pure
``step_plan`` on every branch, the ABI struct, the refusals of the new calls (all made before any HIP call) and the loop override's
pass-through, with no GPU."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _lm_logits_oracle as O
import _lm_loop_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")


# ------------------------------------------------------------------ G23 (a): the stage
def test_g23_oracle_equals_reference_bit_for_bit():
    assert os.path.getsize(O.G23) <= 1 << 20
    cases = O.load_g23_stage()
    assert [c[0].shape for c in cases] == [(3, V) for V in (1, 31, 32, 33, 65, 1003, 2051)]
    n, nans = 0, 0
    for case in cases:
        seen_modes, seen_T, seen_pen = set(), set(), set()
        for setting in case[5]:
            mode, T, pen, want = setting
            assert O.same_bits(O.expected_for(case, setting), want), (case[0].shape, mode, T, pen)
            seen_modes.add(mode), seen_T.add(T), seen_pen.add(pen)
            nans += int(np.isnan(want).sum())
            n += 1
        assert seen_modes == set(O.MODES) and seen_T == {None, 0.7, 0.0} and seen_pen == {1.0, 1.1, 1.3}
    assert n == 5 * 54 + 24 + 6 and nans > 0


def test_g23_holds_the_edge_inputs():
    cases = O.load_g23_stage()
    cond, uncond, _m, _e, hist, sets = cases[4]                  # V = 65: signed zeros, in and out of the history
    assert np.signbit(cond[0, 0]) and np.signbit(uncond[0, 0]) and np.signbit(cond[0, 2]) and not np.signbit(uncond[0, 2])
    assert {0, 2, 4, 6} <= set(hist[0].tolist())
    cond, uncond, *_ = cases[3]                                  # V = 33: -inf - -inf
    assert cond[0, 5] == NEG and uncond[0, 5] == NEG
    for case in cases:                                           # duplicates and pad ids in every history
        h = case[4]
        assert (h[:, 0] == h[:, 1]).all() and (h[:, 3] == h[:, 4]).all()
    # a forced row is -inf off the EOS id, a blocked row -inf on it
    case = cases[5]
    for mode, T, pen, want in case[5]:
        if mode == "force":
            assert np.isinf(np.delete(want, case[3], axis=1)).all() and np.isfinite(want[:, case[3]]).all()
        if mode == "block":
            assert (want[:, case[3]] == NEG).all()


def test_oracle_rules():
    f = np.float32
    c, u = np.array([[1.0, -2.0, 0.5, -0.0]], dtype=f), np.array([[0.25, 1.0, 0.5, 0.0]], dtype=f)
    x = O.shape(c, u, 1.7)
    assert x[0, 0] == f(0.25) + f(1.7) * (f(1.0) - f(0.25)) and x[0, 2] == f(0.5)
    assert O.shape(c)[0].tolist() == c[0].tolist() and np.signbit(O.shape(c)[0, 3])                  # no CFG: untouched, -0.0 kept
    assert not np.signbit(O.shape(c, mask=np.zeros(4, dtype=f))[0, 3])                               # -0.0 + 0.0 = +0.0
    assert O.shape(c, eos_id=1, eos_mode=O.EOS_BLOCK)[0].tolist() == [1.0, NEG, 0.5, -0.0]
    assert O.shape(c, eos_id=1, eos_mode=O.EOS_FORCE)[0].tolist() == [NEG, -2.0, NEG, NEG]
    assert O.shape(c, temperature=0.0)[0, 0] == f(1.0) / f(1e-6)
    seen = O.seen_bitmap([[0, 1, 1, 7, -1]], 4)
    assert seen.tolist() == [[3]]
    assert O.shape(c, penalty=2.0, seen=seen)[0].tolist() == [0.5, -4.0, 0.5, -0.0]
    assert O.seen_bitmap([[31, 32, 64]], 65).tolist() == [[1 << 31, 1, 1]]
    assert O.same_bits([np.nan, 1.0], [np.nan, 1.0]) and not O.same_bits([0.0], [-0.0]) and not O.same_bits([np.nan], [1.0])


# ------------------------------------------------------------------ G23 (b): the loop
@pytest.mark.parametrize("name,B,target,pen,T,seed", L.loop_cases())
def test_loop_restatement_reproduces_the_reference(name, B, target, pen, T, seed):
    want_ids, want_state, want_count = L.load_g23_loop()[name]
    ids, am = L.loop_prompt(B)
    assert am[B:].sum() < am[B:].numel() or B == 1
    model, proc = L.FakeModel(seed), L.make_processor(target, T)
    got = L.run_loop(lambda g, step: model(g if step == 0 else g[:, -1:], torch.ones(g.shape), None if step == 0 else 1).logits[:, 0],
                     L.torch_stage(L.CFG_SCALE, pen), lambda x: torch.argmax(x, dim=-1), ids, L.MAX_NEW, L.EOS, L.PAD, proc)
    assert np.array_equal(got.numpy(), want_ids)
    assert proc.state.name == want_state == "CODES_GENERATION" and proc.codes_count == want_count
    steps = want_ids.shape[1] - ids.shape[1]
    assert want_count == B * steps                                # the count advances by B per step
    if target is not None:
        assert steps == -(-target // B) + 1 and (want_ids[:B, -1] == L.EOS).all()


def test_loop_restatement_with_the_numpy_stage():
    """The same loop with the numpy oracle as its stage: the five steps of ace355_lm_shape are the reference's loop body."""
    name, B, target, pen, T, seed = L.loop_cases()[5]           # B = 2, target 6, penalty 1.3, T 0.85
    want_ids, _s, want_count = L.load_g23_loop()[name]
    ids, _am = L.loop_prompt(B)
    model, proc = L.FakeModel(seed), L.make_processor(target, T)
    mask = proc.non_audio_code_mask[0].numpy()

    def stage(cond, uncond, cur, p):
        if p.state == L.FSMState.THINK_TAG:
            p(cur, torch.zeros(B, L.V_LOOP))                     # the jump, as the reference's __call__ makes it at step 0
        mode = O.EOS_BLOCK if p.codes_count < p.target_codes else O.EOS_FORCE
        return torch.from_numpy(O.shape(cond.numpy(), uncond.numpy(), L.CFG_SCALE, mask, L.EOS, mode, T, pen, O.seen_bitmap(cur.numpy(), L.V_LOOP)))
    got = L.run_loop(lambda g, step: model(g if step == 0 else g[:, -1:], torch.ones(g.shape), None if step == 0 else 1).logits[:, 0],
                     stage, lambda x: torch.argmax(x, dim=-1), ids, L.MAX_NEW, L.EOS, L.PAD, proc)
    assert np.array_equal(got.numpy(), want_ids) and proc.codes_count == want_count


# ------------------------------------------------------------------ step_plan
def _proc(**kw):
    p = L.make_processor(6, 0.85)
    p.metadata_temperature = 0.6
    p.state = L.FSMState.CODES_GENERATION
    p.audio_code_mask = torch.zeros(1, L.V_LOOP)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _view(p, eos=L.EOS, pad=L.PAD, streamer=False, blocked=None):
    from ace355.lmlogits import StepView
    return StepView(p, eos, pad, streamer, blocked)


def test_step_plan_branches():
    from ace355 import native
    from ace355.lmlogits import step_plan
    assert step_plan(_view(None)) == (True, None, native.LM_EOS_NONE, None, False)
    p = _proc(enabled=False)
    assert step_plan(_view(p)) == (True, None, native.LM_EOS_NONE, 0.85, False)
    p.state = L.FSMState.THINK_TAG                               # a disabled processor scales by the metadata temperature there
    assert step_plan(_view(p)) == (True, None, native.LM_EOS_NONE, 0.6, False)
    p = _proc(state=L.FSMState.COMPLETED)
    assert step_plan(_view(p)) == (True, None, native.LM_EOS_NONE, 0.85, False)
    p.generation_phase = "understand"
    plan = step_plan(_view(p))
    assert plan.native and plan.mask is p.audio_code_mask and plan.eos_mode == native.LM_EOS_NONE and not plan.sync_free
    p.audio_code_mask = None
    assert step_plan(_view(p)).mask is None
    p = _proc(state=L.FSMState.THINK_TAG)                        # step 0 of a codes-phase call: the reference's __call__ jumps
    assert step_plan(_view(p)) == (False, None, native.LM_EOS_NONE, None, False)
    p = _proc(state="BPM_VALUE")
    assert not step_plan(_view(p)).native
    p = _proc()
    plan = step_plan(_view(p))
    assert plan.native and plan.mask is p.non_audio_code_mask and plan.eos_mode == native.LM_EOS_BLOCK and plan.temperature == 0.85
    p.codes_count = 6
    assert step_plan(_view(p)).eos_mode == native.LM_EOS_FORCE
    p.codes_count = 5
    assert step_plan(_view(p)).eos_mode == native.LM_EOS_BLOCK
    p.target_codes = None
    assert step_plan(_view(p)).eos_mode == native.LM_EOS_NONE
    p = _proc(eos_token_id=None)
    assert step_plan(_view(p)).eos_mode == native.LM_EOS_NONE
    p = _proc(codes_temperature=None)
    assert step_plan(_view(p)).temperature is None


def test_step_plan_is_pure():
    from ace355.lmlogits import step_plan
    p = _proc()
    before = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in vars(p).items()}
    for streamer in (False, True):
        assert step_plan(_view(p, streamer=streamer)) == step_plan(_view(p, streamer=streamer))
    for k, v in vars(p).items():
        assert torch.equal(v, before[k]) if isinstance(v, torch.Tensor) else v == before[k] or v is before[k], k


def test_step_plan_sync_free_needs_every_clause():
    from ace355.lmlogits import step_plan
    assert step_plan(_view(_proc())).sync_free                    # enabled, CODES_GENERATION, mask, "block", pad -inf, no streamer
    assert step_plan(_view(_proc(), pad=L.EOS)).sync_free         # pad == EOS
    assert step_plan(_view(_proc(), pad=None)).sync_free
    assert step_plan(_view(_proc(), blocked=frozenset({L.PAD}))).sync_free
    assert not step_plan(_view(_proc(enabled=False))).sync_free
    assert not step_plan(_view(_proc(state=L.FSMState.COMPLETED))).sync_free
    assert not step_plan(_view(_proc(non_audio_code_mask=None))).sync_free
    assert not step_plan(_view(_proc(codes_count=6))).sync_free   # "force": the EOS is drawn and must be seen
    assert not step_plan(_view(_proc(target_codes=None))).sync_free
    assert not step_plan(_view(_proc(), pad=400)).sync_free       # an allowed id stops the loop
    assert not step_plan(_view(_proc(), blocked=frozenset())).sync_free
    assert not step_plan(_view(_proc(), streamer=True)).sync_free
    assert not step_plan(_view(_proc(), eos=401)).sync_free       # the loop's EOS is not the processor's, and drawable
    assert step_plan(_view(_proc(), eos=100)).sync_free           # ... or not drawable


# ------------------------------------------------------------------ ABI
def test_shape_params_layout_matches_header(tmp_path):
    from ace355 import native
    ct = native.LmShapeParamsC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ace355.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ace355_lm_shape_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ace355_lm_shape_params, {f}));' for f, _t in ct._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ct) == 40
    assert [f for f, _t in ct._fields_] == ["cfg_scale", "eos_id", "eos_mode", "has_temperature", "temperature", "penalty", "mask", "seen"]
    for f, _t in ct._fields_:
        assert int(got[f]) == getattr(ct, f).offset, f
    assert (native.LM_EOS_NONE, native.LM_EOS_BLOCK, native.LM_EOS_FORCE) == (O.EOS_NONE, O.EOS_BLOCK, O.EOS_FORCE)


SHAPE_REFUSALS = {"B_zero": "B must", "B_large": "B must", "V_zero": "V must", "V_large": "V must", "cond_stride": "stride",
                  "uncond_stride": "stride", "out_stride": "stride", "null_cond": "null", "null_out": "null", "null_params": "null",
                  "eos_low": "eos_id", "eos_high": "eos_id", "eos_mode": "eos_mode", "penalty_zero": "penalty", "penalty_negative": "penalty",
                  "penalty_inf": "penalty", "penalty_nan": "penalty", "null_seen": "seen", "temperature_zero": "temperature"}


@pytest.mark.parametrize("case", list(SHAPE_REFUSALS))
def test_shape_refusals_need_no_gpu(case):
    """Each defect alone is refused with ACE355_ERR_INVALID and a message before any HIP call: the pointers here are not memory."""
    from ace355 import native
    lib = native.lib()
    V = 100
    a = dict(cond=4096, cs=V, uncond=8192, us=V, out=4096, os=V, B=2, V=V)
    p = dict(cfg_scale=2.0, eos_id=5, eos_mode=1, has_temperature=1, temperature=0.85, penalty=1.1, mask=4096, seen=4096)
    null_params = False
    if case == "B_zero":
        a["B"] = 0
    elif case == "B_large":
        a["B"] = native.LM_MAX_SEQS + 1
    elif case == "V_zero":
        a["V"] = 0
    elif case == "V_large":
        a["V"] = a["cs"] = a["us"] = a["os"] = native.LM_PICK_MAX_V + 1
    elif case.endswith("_stride"):
        a[{"cond_stride": "cs", "uncond_stride": "us", "out_stride": "os"}[case]] = V - 1
    elif case == "null_cond":
        a["cond"] = None
    elif case == "null_out":
        a["out"] = None
    elif case == "null_params":
        null_params = True
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
    else:
        p["temperature"] = 0.0
    params = native.LmShapeParamsC(**p)
    lib.ace355_lm_pick_plan(0, None, None)   # leaves another message behind
    rc = lib.ace355_lm_shape(a["cond"], a["cs"], a["uncond"], a["us"], a["out"], a["os"], a["B"], a["V"],
                             None if null_params else ctypes.byref(params), None)
    assert rc == 1 and "lm_shape:" in native.last_error() and SHAPE_REFUSALS[case] in native.last_error(), native.last_error()


@pytest.mark.parametrize("case,word", [("B_zero", "B must"), ("B_large", "B must"), ("V_zero", "V must"), ("V_large", "V must"),
                                       ("T_zero", "T must"), ("T_large", "T must"), ("stride", "row_stride"), ("null_ids", "null"),
                                       ("null_seen", "null")])
def test_seen_mark_refusals_need_no_gpu(case, word):
    from ace355 import native
    lib = native.lib()
    a = dict(ids=4096, stride=9, B=2, T=9, V=100, seen=4096)
    a.update({"B_zero": dict(B=0), "B_large": dict(B=native.LM_MAX_SEQS + 1), "V_zero": dict(V=0), "V_large": dict(V=native.LM_PICK_MAX_V + 1),
              "T_zero": dict(T=0), "T_large": dict(T=native.LM_MAX_POSITIONS + 1, stride=native.LM_MAX_POSITIONS + 1),
              "stride": dict(stride=8), "null_ids": dict(ids=None), "null_seen": dict(seen=None)}[case])
    lib.ace355_lm_pick_plan(0, None, None)
    rc = lib.ace355_lm_seen_mark(a["ids"], a["stride"], a["B"], a["T"], a["V"], a["seen"], None)
    assert rc == 1 and "lm_seen_mark:" in native.last_error() and word in native.last_error(), native.last_error()


def test_decode_tokens_refuses_null_arguments_without_a_gpu():
    """What can be refused without a handle (creating one allocates on the GPU); the refusals that need one are in the GPU tests."""
    from ace355 import native
    lib = native.lib()
    lib.ace355_lm_pick_plan(0, None, None)
    assert lib.ace355_lm_decode_tokens(None, 4096, 1, 4096, None) == 1 and "lm_decode_tokens" in native.last_error()
    assert lib.ace355_lm_bad_tokens(None) == -1


# ------------------------------------------------------------------ the override, where it must not change anything
class _Base:
    def __init__(self):
        self.calls = []

    def _generate_with_cfg_custom(self, *args):
        self.calls.append(args)
        return "reference"


def _handler(flag):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _Base):
        pass

    h = Handler()
    if flag is not None:
        h.use_native_lm_loop = flag
    return h


@pytest.mark.parametrize("flag", [None, False, True])
def test_loop_override_passes_through_when_off_or_on_cpu(flag, monkeypatch, caplog):
    """Flag off (the default without ACE355_LM_LOOP=1), or on with ids on the CPU: the reference's loop gets the very arguments, and
    the native loop is never asked."""
    from ace355 import backend, lmlogits
    if flag is None:
        assert backend.NativeLmMixin.use_native_lm_loop is (os.environ.get("ACE355_LM_LOOP", "") == "1")
        flag = False

    def boom(*a, **k):
        raise AssertionError("the native loop must not be called")
    monkeypatch.setattr(lmlogits, "generate_with_cfg", boom)
    caplog.set_level("INFO", logger="ace355")
    h = _handler(flag)
    h.llm = types.SimpleNamespace()
    ids, am = L.loop_prompt(2)
    proc, streamer = object(), object()
    assert h._generate_with_cfg_custom(ids, am, 12, 0.85, 2.0, None, 0.9, 1.0, L.PAD, streamer, proc) == "reference"
    assert len(h.calls) == 1
    got = h.calls[0]
    assert got[0] is ids and got[1] is am and got[2:9] == (12, 0.85, 2.0, None, 0.9, 1.0, L.PAD) and got[9] is streamer and got[10] is proc
    assert h._lm_loop_stats is None
    # asked for and not possible: said once; not asked for: nothing is said
    assert h._generate_with_cfg_custom(ids, am, 12, 0.85, 2.0, None, 0.9, 1.0, L.PAD, streamer, proc) == "reference"
    said = [r.getMessage() for r in caplog.records if "native-lm-loop" in r.getMessage()]
    assert (len(said) == 1 and "CUDA device" in said[0]) if flag else not said


def test_loop_override_keeps_the_reference_signature():
    import inspect
    from ace355.backend import NativeLmMixin
    names = list(inspect.signature(NativeLmMixin._generate_with_cfg_custom).parameters)
    assert names == ["self", "batch_input_ids", "batch_attention_mask", "max_new_tokens", "temperature", "cfg_scale", "top_k", "top_p",
                     "repetition_penalty", "pad_token_id", "streamer", "constrained_processor"]
