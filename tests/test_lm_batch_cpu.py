"""CPU: the cache fan-out's launch plan (``native.lm_fan_out_plan``, a pure function behind ``ace355_lm_fan_out``) replayed on a numpy
stand-in of the cache, its refusals, and the condition function that decides whether a ``_run_pt`` call runs as one batched loop."""
import ctypes

import numpy as np
import pytest

SRCS = [[0, 0, 1, 1], [0, 0, 0, 1, 1, 1], [0] * 8 + [1] * 8, [0, 1, 2, 3], [0, 1, 1, 2], [0, 0, 1, 2, 3], [0], [0, 0], [0, 1, 2, 2]]


def _n_old(src):
    return max(src) + 1


@pytest.mark.parametrize("src", SRCS, ids=lambda s: "".join(f"{v:x}" for v in s))
def test_fan_out_plan_moves_every_sequence_once_and_never_reads_what_was_written(src):
    from ace355 import native
    waves = native.lm_fan_out_plan(src, _n_old(src))
    copies = [c for w in waves for c in w]
    assert all(w for w in waves)                                                         # no empty launch
    assert sorted(d for d, _s in copies) == [n for n, s in enumerate(src) if s != n]     # every destination that moves, once
    assert all(s == src[d] for d, s in copies)
    written = set()
    for w in waves:
        written |= {d for d, _s in w}                                                    # the wave's own writes count too
        assert not written & {s for _d, s in w}, (src, waves)


@pytest.mark.parametrize("src", SRCS, ids=lambda s: "".join(f"{v:x}" for v in s))
def test_fan_out_plan_replayed_in_place_equals_a_gather(src):
    from ace355 import native
    n_old = _n_old(src)
    old = np.random.default_rng(len(src)).standard_normal((16, 5)).astype(np.float32)
    cache = old.copy()
    for w in native.lm_fan_out_plan(src, n_old):
        for d, s in w:                                                                   # one launch: copies in any order
            cache[d] = cache[s]
    assert np.array_equal(cache[:len(src)], old[src])
    assert np.array_equal(cache[len(src):], old[len(src):])


def test_fan_out_plan_of_the_hazard_case_is_two_waves():
    from ace355 import native
    assert native.lm_fan_out_plan([0, 0, 1, 1], 2) == [[(2, 1), (3, 1)], [(1, 0)]]
    assert native.lm_fan_out_plan([0] * 8 + [1] * 8, 2) == [[(n, n // 8) for n in range(2, 16)], [(1, 0)]]
    assert native.lm_fan_out_plan([0, 1, 2], 3) == []
    assert len(native.lm_fan_out_plan([0] + list(range(15)), 15)) == 15       # [0, 0, 1, .. 14]: the longest chain


@pytest.mark.parametrize("src,n_old,text", [([0, 1, 0], 2, "non-decreasing"), ([1, 1], 2, "[0, n]"), ([0, 2, 2], 3, "[0, n]"),
                                            ([-1, 0], 2, "[0, n]"), ([0, 1, 2], 2, "does not hold"), ([0, 0], 0, "1 .. 16"),
                                            ([0] * 17, 1, "1 .. 16"), ([], 1, "1 .. 16")])
def test_fan_out_plan_refusals(src, n_old, text):
    from ace355 import native
    with pytest.raises(RuntimeError, match="lm_fan_out_plan"):
        native.lm_fan_out_plan(src, n_old)
    assert text in native.last_error()


def test_fan_out_refuses_a_null_handle_before_any_hip_call():
    from ace355 import native
    src = (ctypes.c_int32 * 2)(0, 0)
    assert native.lib().ace355_lm_fan_out(None, src, 2, None) == 1 and "lm_fan_out" in native.last_error()


# ------------------------------------------------------------------ a sequence's launches do not see the batch
@pytest.mark.parametrize("dims", [(1024, 3072, 16, 8), (2048, 6144, 16, 8), (256, 768, 4, 2)], ids=["0.6B", "1.7B", "tiny"])
def test_a_decode_step_plans_the_same_launches_for_2_to_16_sequences(dims):
    """Why song i of a batched loop can equal the loop run alone: apart from the row count, a decode step over N sequences is the
    same list of launches for N = 2 .. 16, and every projection gets the same GEMM plan (tile, split-K, K rotation)."""
    from ace355 import native

    def step(N):
        p = native.encoder_pass_plan(*dims, 2, N, 1, causal=1, has_cache=1, pos0=512, max_pos=2048, max_seqs=16, has_first=1)
        return [{k: v for k, v in s.items() if k not in ("M", "seqs", "flops")} for s in p["steps"]], \
               [native.gemm_plan(s["M"], s["N"], s["K"], s["mode"]) for s in p["steps"] if s["kind"] == "gemm"]

    launches, plans = step(2)
    assert len(plans) == 8 and all(p["ksplit"] == 1 and p["kparts"] == 1 for p in plans)
    for N in range(3, 17):
        assert step(N) == (launches, plans), N


# ------------------------------------------------------------------ the seam's conditions
GOOD = dict(formatted_prompts=["p", "p", "p"], cfg_scale=2.0, generation_phase="codes", use_constrained_decoding=True,
            target_duration=30.0, seeds=[1, 2, 3])


def test_batch_request_accepts_the_reference_batch_call():
    from ace355.lmlogits import batch_request
    assert batch_request(**GOOD) == (True, None)
    assert batch_request(**{**GOOD, "seeds": (4, 5, 6, 7)}) == (True, None)


@pytest.mark.parametrize("change,text", [
    ({"formatted_prompts": "p"}, "not a list"), ({"formatted_prompts": ["p"]}, "not a list"),
    ({"formatted_prompts": ["p", "p", "q"]}, "differ"),
    ({"cfg_scale": 1.0}, "cfg_scale"),
    ({"generation_phase": "cot"}, "phase"),
    ({"use_constrained_decoding": False}, "constrained decoding"),
    ({"target_duration": None}, "target duration"), ({"target_duration": 0}, "target duration"),
    ({"seeds": None}, "seeds"), ({"seeds": [1, 2]}, "seeds"), ({"seeds": [1, None, 3]}, "seeds"), ({"seeds": [1, 2.0, 3]}, "seeds"),
    ({"loop_refusal": "4 sequences exceed the native handle"}, "exceed the native handle")])
def test_each_condition_alone_sends_the_call_to_the_sequential_path(change, text):
    from ace355.lmlogits import batch_request
    ok, why = batch_request(**{**GOOD, **change})
    assert ok is False and text in why


def test_run_pt_passes_through_with_the_flag_off_or_a_condition_unmet(caplog):
    """No GPU: with the flag off nothing is looked at; with it on, a call that misses a condition reaches the host's ``_run_pt``
    with its arguments, and says why once."""
    import logging
    from ace355.backend import NativeLmMixin

    class Host:
        def _run_pt(self, formatted_prompts, *a, **k):
            return ("host", formatted_prompts, a, k["seeds"])

    class Handler(NativeLmMixin, Host):
        pass

    h = Handler()
    assert Handler.use_native_lm_batch is False
    args = (0.85, 2.0, "NO USER INPUT", None, 0.9, 1.0)
    assert h._run_pt(["p", "p"], *args, generation_phase="codes", target_duration=30.0, seeds=[1, 2]) == ("host", ["p", "p"], args, [1, 2])
    h.use_native_lm_batch = True
    with caplog.at_level(logging.INFO, logger="ace355"):
        for _ in range(2):
            assert h._run_pt(["p", "q"], *args, generation_phase="codes", target_duration=30.0, seeds=[1, 2])[0] == "host"
        assert h._run_pt(["p", "p"], *args, generation_phase="codes", target_duration=30.0, seeds=None)[0] == "host"
    said = [r.getMessage() for r in caplog.records if "[native-lm-batch]" in r.getMessage()]
    assert len(said) == 2 and "differ" in said[0] and "seeds" in said[1]
