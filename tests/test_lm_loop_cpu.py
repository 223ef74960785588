"""CPU: the control flow of the 5 Hz LM's CFG loops - ``generate_with_cfg`` and ``generate_codes_batch``, the production functions - on
stand-ins for the LM, the logits stage and the selection (tests/_lm_loop_stubs.py): the recorded reference loops of G23, song i of a
batch against the sequential loop seeded ``seeds[i]``, the streamer, the bad-draw epilogue and the batched loop's refusals."""
import numpy as np
import pytest
import torch

import _lm_loop_ref as R
import _lm_loop_stubs as St

TEMP, TOP_P, CFG = 0.85, 0.9, 2.0
SEEDS = [3, 11, 3, 29]


def _lm_calls(log):
    return [c for c in log if c in ("prefill", "decode_tokens", "fan_out", "bad_tokens")]


# ------------------------------------------------------------------ 1. the single loop reproduces the recorded reference loops
@pytest.mark.parametrize("name,B,target,pen,T,seed", R.loop_cases())
def test_single_loop_reproduces_the_recorded_reference_loops(monkeypatch, name, B, target, pen, T, seed):
    from ace355.lmlogits import generate_with_cfg
    log = St.install(monkeypatch, St.argmax_pick)
    want_ids, want_state, want_count = R.load_g23_loop()[name]
    ids, am = R.loop_prompt(B)
    proc, h, lm = R.make_processor(target, T), St.StubHandler(), St.StubLm(seed, log)
    got = generate_with_cfg(h, lm, ids, am, R.MAX_NEW, 0.0, R.CFG_SCALE, None, None, pen, R.PAD, None, proc)
    assert got.dtype == ids.dtype and np.array_equal(got.numpy(), want_ids)
    assert proc.state.name == want_state and proc.codes_count == want_count
    stats = h._lm_loop_stats
    steps = want_ids.shape[1] - ids.shape[1]
    assert set(stats) == {"steps", "native_steps", "sync_free_steps", "token_reads"} and stats["steps"] == steps
    assert stats["native_steps"] == steps - 1                     # step 0 is the reference's processor (THINK_TAG -> CODES_GENERATION)
    if target is not None:
        assert stats["token_reads"] == 2 and stats["sync_free_steps"] == stats["native_steps"] - 1
    else:
        assert stats["sync_free_steps"] == 0 and stats["token_reads"] == steps
    # one forward per step between the two bad_tokens reads; every step: stage, selection, then the bitmap
    assert _lm_calls(log) == ["bad_tokens", "prefill"] + ["decode_tokens"] * (steps - 1) + ["bad_tokens"]
    marks = ["mark"] if pen != 1.0 else []
    body = [c for c in log if c not in ("prefill", "decode_tokens", "bad_tokens")]
    assert body == marks + ["select"] + marks + (["shape", "pick"] + marks) * (steps - 1)
    assert lm.fed == [want_ids[:B, ids.shape[1] + t].tolist() for t in range(steps - 1)]


# ------------------------------------------------------------------ 2. song i of a batch is the sequential loop seeded seeds[i]
def _sequential(monkeypatch, seed, target, pen, T, max_new, start_in_codes):
    from ace355.lmlogits import generate_with_cfg
    log = St.install(monkeypatch, St.oracle_pick)
    ids, am = R.loop_prompt(1)
    proc, h = R.make_processor(target, T), St.StubHandler()
    if start_in_codes:
        proc.state = R.FSMState.CODES_GENERATION
    torch.manual_seed(seed)
    out = generate_with_cfg(h, St.StubLm(7, log, St.role_logits), ids, am, max_new, TEMP, CFG, None, TOP_P, pen, R.PAD, None, proc)
    return out[0], proc


@pytest.mark.parametrize("target,pen,T,start_in_codes", [(6, 1.0, None, False), (10, 2.0, 0.5, False), (6, 1.3, 0.85, True)],
                         ids=["t6_plain", "t10_penalty2_T0.5", "t6_native_step0"])
def test_batched_loop_rows_equal_the_sequential_loop_per_seed(monkeypatch, target, pen, T, start_in_codes):
    """(The third case starts in CODES_GENERATION, so that step 0 is a native step: the pair's staged row is repeated before the stage.)"""
    from ace355.lmlogits import generate_codes_batch
    seq = [_sequential(monkeypatch, s, target, pen, T, 14, start_in_codes) for s in SEEDS]
    want = torch.stack([row for row, _p in seq])
    log = St.install(monkeypatch, St.oracle_pick)
    ids, am = R.loop_prompt(1)
    proc, h, lm = R.make_processor(target, T), St.StubHandler(), St.StubLm(7, log, St.role_logits)
    if start_in_codes:
        proc.state = R.FSMState.CODES_GENERATION
    torch.manual_seed(1234)
    rng = torch.get_rng_state()
    got = generate_codes_batch(h, lm, ids, am, SEEDS, 14, TEMP, CFG, None, TOP_P, pen, R.PAD, proc)
    assert torch.equal(torch.get_rng_state(), rng)                # the global generator is not touched
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(got[0], got[2]) and len({tuple(r.tolist()) for r in got}) == 3
    steps = target + 1
    assert got.shape == (4, 6 + steps) and (got[:, -1] == R.EOS).all()
    assert proc.codes_count == seq[-1][1].codes_count == steps and proc.state == seq[-1][1].state == R.FSMState.CODES_GENERATION
    stats = h._lm_loop_stats
    assert stats["batch"] == 4 and stats["prefill_rows"] == 2 and stats["steps"] == steps
    native0 = 1 if start_in_codes else 0
    assert stats["native_steps"] == steps - 1 + native0 and stats["sync_free_steps"] == steps - 2 + native0
    assert stats["token_reads"] == 2 - native0
    # the fan-out: once, after step 0's tokens are selected and before the first decode
    assert lm.fan_outs == [[0] * 4 + [1] * 4]
    assert _lm_calls(log) == ["bad_tokens", "prefill", "fan_out"] + ["decode_tokens"] * (steps - 1) + ["bad_tokens"]
    assert log.index("pick") < log.index("fan_out") < log.index("decode_tokens") and "select" not in log
    assert lm.fed == [got[:, 6 + t].tolist() for t in range(steps - 1)]


# ------------------------------------------------------------------ 3. the streamer, and a step that can draw no token
def _single(monkeypatch, B, target, max_new, streamer, nan_step=None, processor=True):
    from ace355.lmlogits import generate_with_cfg
    log = St.install(monkeypatch, St.argmax_pick)
    ids, am = R.loop_prompt(B)
    proc = R.make_processor(target, None) if processor else None
    h, lm = St.StubHandler(), St.StubLm(2304, log, nan_step=nan_step)
    run = lambda: generate_with_cfg(h, lm, ids, am, max_new, 0.0, R.CFG_SCALE, None, None, 1.0, R.PAD, streamer, proc)   # noqa: E731
    return run, h, lm, proc


def test_single_loop_with_a_streamer_puts_every_step_and_ends_once(monkeypatch):
    s = St.Streamer()
    run, h, _lm, proc = _single(monkeypatch, 2, 6, R.MAX_NEW, s)
    got = run()
    want_ids, _state, want_count = R.load_g23_loop()["B2_t6_p1.0"]
    assert np.array_equal(got.numpy(), want_ids) and proc.codes_count == want_count
    stats = h._lm_loop_stats
    assert stats["steps"] == 4 and stats["sync_free_steps"] == 0 and stats["token_reads"] == 4
    assert s.ended == 1 and len(s.put_calls) == 4
    assert all(p.shape == (2, 1) and torch.equal(p[:, 0], got[:2, 6 + t]) for t, p in enumerate(s.put_calls))


@pytest.mark.parametrize("processor", [True, False], ids=["target6", "no_processor"])
def test_single_loop_ends_the_streamer_before_it_raises_for_a_bad_draw(monkeypatch, processor):
    """A NaN in step 2's logits: the step reads its tokens (a streamer is there), finds -1 and stops the loop there."""
    s = St.Streamer()
    run, h, lm, proc = _single(monkeypatch, 2, 6, R.MAX_NEW, s, nan_step=2, processor=processor)
    with pytest.raises(RuntimeError, match="no valid token"):
        run()
    assert s.ended == 1 and len(s.put_calls) == 2                # the bad step's tokens are not put
    assert h._lm_loop_stats["steps"] == 3 and h._lm_loop_stats["token_reads"] == 3 and len(lm.fed) == 2
    assert proc is None or proc.codes_count == 4                 # the bad step's tokens do not reach the processor


def test_single_loop_without_a_processor_stops_at_the_bad_draw(monkeypatch):
    run, h, lm, _p = _single(monkeypatch, 2, None, 6, None, nan_step=2, processor=False)
    with pytest.raises(RuntimeError, match=r"no valid token .*0 ids replaced.* advanced 3 steps"):
        run()
    assert h._lm_loop_stats["steps"] == 3 and len(lm.fed) == 2


def test_single_loop_runs_on_through_a_sync_free_bad_draw_and_raises_after_it(monkeypatch):
    """With a 40-code target the steps after step 0 read nothing: the -1 is fed on as data and the check after the loop raises."""
    run, h, lm, proc = _single(monkeypatch, 2, 40, 6, None, nan_step=2)
    with pytest.raises(RuntimeError, match=r"no valid token .* advanced 6 steps"):
        run()
    stats = h._lm_loop_stats
    assert stats["steps"] == 6 and stats["token_reads"] == 1 and stats["sync_free_steps"] == 5 and proc.codes_count == 2 * 6
    assert lm.fed[2][0] == -1 and 300 <= lm.fed[2][1] < 900


# ------------------------------------------------------------------ 4. what the batched loop refuses, and when it raises
def _batched(monkeypatch, proc, seeds=SEEDS, ids=None, eos=R.EOS, boost=None, max_new=14):
    from ace355.lmlogits import generate_codes_batch
    log = St.install(monkeypatch, St.oracle_pick)
    pair, am = R.loop_prompt(1)
    if ids is not None:
        pair, am = ids, None
    h, lm = St.StubHandler(eos), St.StubLm(7, log, St.role_logits, boost=boost)
    return (lambda: generate_codes_batch(h, lm, pair, am, seeds, max_new, TEMP, CFG, None, TOP_P, 1.0, R.PAD, proc)), h, lm, log


@pytest.mark.parametrize("change", [{"target_codes": None}, {"enabled": False}, {"eos_token_id": None}, None])
def test_batched_loop_needs_a_processor_that_ends_every_song_together(monkeypatch, change):
    proc = None
    if change is not None:
        proc = R.make_processor(6, None)
        for k, v in change.items():
            setattr(proc, k, v)
    run, _h, _lm, log = _batched(monkeypatch, proc)
    with pytest.raises(RuntimeError, match="needs an enabled constrained processor with target_codes and eos_token_id"):
        run()
    assert log == []


def test_batched_loop_refuses_more_songs_than_the_handle_holds_and_a_wrong_pair(monkeypatch):
    run, _h, _lm, log = _batched(monkeypatch, R.make_processor(6, None), seeds=list(range(9)))
    with pytest.raises(ValueError, match="9 songs need 18 sequences, the native LM holds 16"):
        run()
    run, _h, _lm, _log = _batched(monkeypatch, R.make_processor(6, None), seeds=[])
    with pytest.raises(ValueError, match="0 songs need 0 sequences"):
        run()
    for bad in (R.loop_prompt(2)[0], R.loop_prompt(1)[0][0], R.loop_prompt(1)[0][:1]):
        run, _h, _lm, log = _batched(monkeypatch, R.make_processor(6, None), ids=bad)
        with pytest.raises(ValueError, match=r"takes the \[2, P\] pair"):
            run()
        assert log == []


def test_batched_loop_raises_when_only_some_rows_stop(monkeypatch):
    """The tokenizer's EOS is an id the codes mask allows (the processor blocks another): step 2's logits push it on song 1 only."""
    stop = 500
    run, h, lm, _log = _batched(monkeypatch, R.make_processor(40, None), eos=stop, boost=(2, 1, stop), max_new=8)
    with pytest.raises(RuntimeError, match=r"songs \[1\] of 4 stopped at step 2 and the others did not; the batched LM loop returns no ragged rows"):
        run()
    assert h._lm_loop_stats["sync_free_steps"] == 0 and h._lm_loop_stats["token_reads"] == 3 and len(lm.fed) == 2


class _LeavingProcessor(R.CodesProcessor):
    """Leaves CODES_GENERATION for ``to`` at its ``at``-th count."""

    def __init__(self, at, to, target):
        super().__init__(R.V_LOOP, R.ALLOWED, R.EOS, target_codes=target)
        self.at, self.to = at, to

    def update_state(self, token):
        super().update_state(token)
        if self.codes_count == self.at:
            self.state = self.to


def test_batched_loop_raises_when_the_processor_leaves_the_codes_phase(monkeypatch):
    run, _h, lm, _log = _batched(monkeypatch, _LeavingProcessor(1, R.FSMState.COMPLETED, 40))      # seen right after step 0's read
    with pytest.raises(RuntimeError, match="is in state COMPLETED after step 0 of a batched loop; only the codes phase runs batched"):
        run()
    assert lm.fan_outs == [[0] * 4 + [1] * 4] and lm.fed == []
    run, h, lm, _log = _batched(monkeypatch, _LeavingProcessor(3, R.FSMState.THINK_TAG, 40))       # on a sync-free step: seen by the next plan
    with pytest.raises(RuntimeError, match=r"left the codes phase at step 3 of a batched loop \(state THINK_TAG\)"):
        run()
    assert h._lm_loop_stats["sync_free_steps"] == 2 and len(lm.fed) == 3
