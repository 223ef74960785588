"""GPU: the cache fan-out keeps a sequence's bits (in place, across the decode attention's chunk split, after decode steps), its
refusals leave the handle alone, ``generate_codes_batch`` gives every song the tokens of the sequential native loop for its seed, and
``NativeLmMixin._run_pt`` returns the sequential path's strings from one batched loop."""
import ctypes as C
import logging

import pytest
import torch

import _lm_batch_ref as S
import _lm_loop_ref as R
import _lm_oracle as L

pytestmark = pytest.mark.gpu

V = L.TINY.vocab_size
TOP_P, TEMP, CFG = 0.9, 0.85, 2.0
SEEDS = [101, 202, 303, 404, 505, 606, 707, 808]


@pytest.fixture(scope="module")
def lm(gpu_device):
    from ace355.lm import NativeCausalLM
    lm = NativeCausalLM(L.TINY, gpu_device, max_positions=72, max_seqs=16)
    lm.load_state_dict(dict(L.weights("tiny")))
    yield lm
    lm.close()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pair(P, seed):
    """ids and mask [2, P], first = [0, 2]."""
    ids, first = L.left_padded([P, P - 2], P, V, seed)
    return ids, L.mask_of(first, P)


def _tokens(k, n, seed):
    return torch.randint(0, V, (k, n), generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ fan-out keeps bits
@pytest.mark.parametrize("P,k,copies", [(6, 4, 2), (60, 10, 3)], ids=["in_place_hazard", "across_the_chunk_split"])
def test_fan_out_keeps_the_bits_of_every_sequence(lm, P, k, copies):
    """[0, 0, 1, 1]: destination 1 overwrites old sequence 1 while 2 and 3 still read it.  P = 60 running to 70 crosses the decode
    attention's 64 | 65 chunk split.  The first copy of each old sequence is fed run A's tokens and must give run A's bits; the others
    are fed other tokens and must not."""
    ids, am = _pair(P, 40 + P)
    a_tok, other = _tokens(k, 2, 41), _tokens(k, 2, 42)
    lm.prefill(ids, am)
    want = [lm.decode(a_tok[t]) for t in range(k)]
    assert lm.length == P + k

    lm.prefill(ids, am)
    lm.fan_out([0] * copies + [1] * copies)
    assert lm.length == P and lm._first == [0] * copies + [2] * copies
    for t in range(k):
        fed = torch.cat([a_tok[t, :1], other[t, :1].expand(copies - 1), a_tok[t, 1:], other[t, 1:].expand(copies - 1)])
        got = lm.decode(fed)
        assert got.shape == (2 * copies, V)
        assert torch.equal(_bits(got[0]), _bits(want[t][0])) and torch.equal(_bits(got[copies]), _bits(want[t][1])), t
        for r in range(1, copies):
            assert not torch.equal(_bits(got[r]), _bits(want[t][0])) and not torch.equal(_bits(got[copies + r]), _bits(want[t][1])), t
    assert lm.length == P + k


def test_fan_out_after_decode_steps_copies_the_whole_length(lm, gpu_device):
    """A fan-out at length P + 3 must carry the three decoded rows too: every copy, fed run A's tokens, gives run A's bits, through
    ``decode`` and through ``decode_tokens``."""
    P, k = 6, 4
    ids, am = _pair(P, 50)
    a_tok = _tokens(3 + k, 2, 51)
    lm.prefill(ids, am)
    want = [lm.decode(a_tok[t]) for t in range(3 + k)]

    lm.prefill(ids, am)
    for t in range(3):
        lm.decode(a_tok[t])
    lm.fan_out([0, 0, 1, 1])
    assert lm.length == P + 3
    for t in range(3, 3 + k):
        got = lm.decode(a_tok[t].repeat_interleave(2)) if t % 2 else lm.decode_tokens(a_tok[t].repeat_interleave(2).to(gpu_device))
        for r in range(4):
            assert torch.equal(_bits(got[r]), _bits(want[t][r // 2])), (t, r)
    assert lm.bad_tokens() == 0

    lm.prefill(ids, am)                                          # and a fan-out that drops a sequence, then one that widens again
    lm.fan_out([0])
    assert lm._first == [0] and lm.length == P
    lm.fan_out([0, 0, 0])
    got = lm.decode(a_tok[0, :1].expand(3))
    for r in range(3):
        assert torch.equal(_bits(got[r]), _bits(want[0][0]))


# ------------------------------------------------------------------ refusals
def test_fan_out_refusals_leave_the_handle_alone(gpu_device):
    from ace355 import native
    from ace355.lm import NativeCausalLM
    lib = native.lib()
    small = NativeCausalLM(L.TINY, gpu_device, max_positions=16, max_seqs=4)
    try:
        small.load_state_dict(dict(L.weights("tiny")))

        def raw(src):
            return lib.ace355_lm_fan_out(small._h, (C.c_int32 * len(src))(*src), len(src), None)

        assert raw([0, 0]) == 1 and "no prefill" in native.last_error() and small.length == 0
        with pytest.raises(ValueError):
            small.fan_out([0, 0])
        ids, am = _pair(6, 60)
        nxt = torch.tensor([5, 900])
        small.prefill(ids, am)
        want = small.decode(nxt)
        small.prefill(ids, am)
        for src, text in (([0, 0, 0, 1, 1], "max_seqs"), ([], "max_seqs"), ([0, 1, 0], "non-decreasing"), ([1, 1], "[0, n]"),
                          ([0, 1, 2], "does not hold"), ([-1, 0], "[0, n]")):
            assert raw(src) == 1 and text in native.last_error(), src
            with pytest.raises(ValueError):
                small.fan_out(src)
        assert small.length == 6 and small._first == [0, 2]
        assert torch.equal(_bits(small.decode(nxt)), _bits(want))
    finally:
        small.close()


# ------------------------------------------------------------------ the loop
def _loop_handler(lm, gpu_device):
    return S.make_handler(lm, gpu_device)


def _prompt(gpu_device):
    ids, am = R.loop_prompt(1)
    return ids.to(gpu_device), am.to(gpu_device)


_SEQUENTIAL = {}


def _sequential_row(lm, gpu_device, seed, target, pair, temperature=TEMP):
    """The conditional row of the B = 1 native loop after ``torch.manual_seed(seed)`` with a fresh processor: computed once per case."""
    key = (seed if temperature > 0 else None, target, pair, temperature)
    if key not in _SEQUENTIAL:
        pen, T = (2.0, 0.5) if pair else (1.0, None)
        ids, am = _prompt(gpu_device)
        h, proc = _loop_handler(lm, gpu_device), R.make_processor(target, T)
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        out = h._generate_with_cfg_custom(ids, am, target + 10, temperature, CFG, None, TOP_P, pen, R.PAD, None, proc)
        assert proc.codes_count == target + 1 and h._lm_loop_stats["steps"] == target + 1
        _SEQUENTIAL[key] = out[0].cpu()
    return _SEQUENTIAL[key]


def _batched(lm, gpu_device, seeds, target, pair, temperature=TEMP):
    from ace355.lmlogits import generate_codes_batch
    pen, T = (2.0, 0.5) if pair else (1.0, None)
    ids, am = _prompt(gpu_device)
    h, proc = _loop_handler(lm, gpu_device), R.make_processor(target, T)
    out = generate_codes_batch(h, lm, ids, am, seeds, target + 10, temperature, CFG, None, TOP_P, pen, R.PAD, proc)
    return out, h._lm_loop_stats, proc


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "penalty2_T0.5"])
@pytest.mark.parametrize("target", [6, 10])
@pytest.mark.parametrize("B", [2, 3, 8])
def test_every_song_equals_the_sequential_loop_for_its_seed(lm, gpu_device, B, target, pair):
    seeds = SEEDS[:B]
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(gpu_device)
    got, stats, proc = _batched(lm, gpu_device, seeds, target, pair)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(gpu_device), gpu_state)
    assert lm.length == 6 + target and len(lm._first) == 2 * B
    want = torch.stack([_sequential_row(lm, gpu_device, s, target, pair) for s in seeds])
    assert got.dtype == torch.int64 and got.device == gpu_device and got.shape == (B, 6 + target + 1)
    assert torch.equal(got.cpu(), want)
    assert (got[:, -1] == R.EOS).all() and ((got[:, 6:-1] >= 300) & (got[:, 6:-1] < 900)).all()
    assert len({tuple(r.tolist()) for r in got.cpu()}) > 1       # the seeds do steer the songs
    assert stats["steps"] == target + 1 and stats["token_reads"] <= 2 and stats["batch"] == B and stats["prefill_rows"] == 2
    assert stats["native_steps"] == target and stats["sync_free_steps"] == target - 1
    assert proc.codes_count == target + 1 and proc.state == R.FSMState.CODES_GENERATION


def test_equal_seeds_give_equal_songs_and_greedy_gives_one_song(lm, gpu_device):
    got, _stats, _proc = _batched(lm, gpu_device, [707, 202, 707], 6, True)
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    assert torch.equal(got[1].cpu(), _sequential_row(lm, gpu_device, 202, 6, True))
    got, stats, proc = _batched(lm, gpu_device, [1, 2, 3, 4], 6, True, temperature=0.0)
    assert all(torch.equal(got[0], r) for r in got[1:])
    assert torch.equal(got[0].cpu(), _sequential_row(lm, gpu_device, 1, 6, True, temperature=0.0))
    assert stats["steps"] == 7 and proc.codes_count == 7


def test_a_processor_that_cannot_end_the_songs_together_is_refused_before_any_launch(gpu_device):
    from ace355.lmlogits import generate_codes_batch
    ids, am = _prompt(gpu_device)

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the LM was asked for {name}")

    h = _loop_handler(Untouchable(), gpu_device)
    off = R.make_processor(6, None)
    off.enabled = False
    for proc in (None, R.make_processor(None, None), off):
        with pytest.raises(RuntimeError, match="target_codes"):
            generate_codes_batch(h, h.llm, ids, am, [1, 2], 16, TEMP, CFG, None, TOP_P, 1.0, R.PAD, proc)


class _TwoIdLm:
    """What generate_codes_batch asks of a NativeCausalLM, with prefill logits that leave two ids to draw from: 301 with probability
    ``p`` and the pad id with 1 - p (conditional = unconditional, so CFG changes nothing)."""
    out_dtype, cfg, max_seqs = torch.float32, L.TINY, 16

    def __init__(self, dev, p):
        self.dev, self.p, self.fanned, self.decodes = dev, p, None, 0

    def prefill(self, ids, mask):
        x = torch.zeros(2, V, device=self.dev)
        x[:, 301], x[:, R.PAD] = torch.log(torch.tensor(self.p)), torch.log(torch.tensor(1.0 - self.p))
        return x

    def fan_out(self, src):
        self.fanned = list(src)

    def decode_tokens(self, tokens):
        self.decodes += 1
        raise AssertionError("the loop went on after a ragged step")

    def bad_tokens(self):
        return 0


def test_rows_that_do_not_stop_together_raise(gpu_device):
    """A mask that lets the pad id through: at step 0, which reads its tokens, the songs whose uniform falls on the pad id's side of
    ``p`` stop and the others do not.  The selection walks the ids in ascending order, so u < p draws 301; ``p`` is put in the
    widest gap between the songs' first uniforms, so both sides are taken.  The loop raises instead of returning ragged rows."""
    from ace355.lmlogits import generate_codes_batch
    ids, am = _prompt(gpu_device)
    seeds = SEEDS[:4]
    u = sorted(float(torch.rand(1, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(s))) for s in seeds)
    gap, lo = max((b - a, a) for a, b in zip(u, u[1:]))
    assert gap > 1e-3
    stub = _TwoIdLm(gpu_device, lo + gap / 2)
    h = _loop_handler(stub, gpu_device)
    proc = R.CodesProcessor(R.V_LOOP, [R.PAD, 301], R.EOS, target_codes=6)
    with pytest.raises(RuntimeError, match="ragged"):
        generate_codes_batch(h, stub, ids, am, seeds, 16, 1.0, CFG, None, None, 1.0, R.PAD, proc)
    assert stub.fanned == [0] * 4 + [1] * 4 and stub.decodes == 0 and h._lm_loop_stats["token_reads"] == 1


# ------------------------------------------------------------------ the seam
ARGS = dict(temperature=TEMP, cfg_scale=CFG, negative_prompt="NO USER INPUT", top_k=None, top_p=TOP_P, repetition_penalty=2.0,
            use_constrained_decoding=True, target_duration=1.2, generation_phase="codes", caption="c", lyrics="l", cot_text="t")


def _sequential_texts(lm, gpu_device, seeds):
    h = S.make_handler(lm, gpu_device, codes_temperature=None, batch=False)
    texts = h._run_pt([S.COND_PROMPT] * len(seeds), seeds=list(seeds), **ARGS)
    assert h.calls == len(seeds) and h._lm_loop_stats["steps"] == 7 and "batch" not in h._lm_loop_stats
    return texts


def test_run_pt_batched_returns_the_sequential_strings(lm, gpu_device, caplog):
    seeds = SEEDS[:3]
    want = _sequential_texts(lm, gpu_device, seeds)
    h = S.make_handler(lm, gpu_device)
    h.use_native_lm_loop = False                                 # the batched path implies the native loop
    with caplog.at_level(logging.INFO, logger="ace355"):
        got = h._run_pt([S.COND_PROMPT] * 3, seeds=list(seeds), **ARGS)
    assert got == want and len(set(got)) > 1 and all(t.endswith(str(R.EOS)) and len(t.split()) == 7 for t in got)
    assert h.calls == 0 and h._lm_loop_stats["batch"] == 3 and h._lm_loop_stats["prefill_rows"] == 2
    assert not [r for r in caplog.records if "native-lm-batch" in r.getMessage()]
    assert h.setups == [(None, False, True, True, True, False)] and h.contexts == 1
    assert h.llm_tokenizer.sides == ["left"] and h.llm_tokenizer.padding_side == "right"
    assert h.constrained_processor.codes_count == 7


def test_run_pt_batched_runs_more_items_than_the_handle_holds_as_groups(gpu_device):
    from ace355.lm import NativeCausalLM
    small = NativeCausalLM(L.TINY, gpu_device, max_positions=32, max_seqs=4)
    try:
        small.load_state_dict(dict(L.weights("tiny")))
        seeds = SEEDS[:5]
        want = _sequential_texts(small, gpu_device, seeds)
        h = S.make_handler(small, gpu_device)
        assert h._run_pt([S.COND_PROMPT] * 5, seeds=list(seeds), **ARGS) == want
        assert h.calls == 0 and len(h.setups) == 3 and h._lm_loop_stats["batch"] == 1      # groups of 2, 2 and 1
    finally:
        small.close()


def test_run_pt_goes_sequential_when_not_asked_or_not_a_batch_of_one_prompt(lm, gpu_device, caplog):
    seeds = SEEDS[:2]
    want = _sequential_texts(lm, gpu_device, seeds)
    caplog.set_level(logging.INFO, logger="ace355")
    h = S.make_handler(lm, gpu_device, batch=False)              # the flag off
    assert h._run_pt([S.COND_PROMPT] * 2, seeds=list(seeds), **ARGS) == want and h.calls == 2
    assert not [r for r in caplog.records if "native-lm-batch" in r.getMessage()]
    h = S.make_handler(lm, gpu_device)
    other = S.COND_PROMPT.replace("11", "15")
    got = h._run_pt([S.COND_PROMPT, other], seeds=list(seeds), **ARGS)                     # unequal prompts
    assert h.calls == 2 and got[0] == want[0] and "batch" not in h._lm_loop_stats
    h = S.make_handler(lm, gpu_device)
    assert len(h._run_pt([S.COND_PROMPT] * 2, seeds=None, **ARGS)) == 2 and h.calls == 2    # no seeds
    said = [r.getMessage() for r in caplog.records if "native-lm-batch" in r.getMessage()]
    assert len(said) == 2 and "differ" in said[0] and "seeds" in said[1]


def test_run_pt_falls_back_when_the_native_part_fails(lm, gpu_device, caplog, monkeypatch):
    seeds = SEEDS[:2]
    want = _sequential_texts(lm, gpu_device, seeds)

    def broken(src):
        raise RuntimeError("fan-out stub: no")

    monkeypatch.setattr(lm, "fan_out", broken, raising=False)
    h = S.make_handler(lm, gpu_device)
    with caplog.at_level(logging.WARNING, logger="ace355"):
        got = h._run_pt([S.COND_PROMPT] * 2, seeds=list(seeds), **ARGS)
    assert got == want and h.calls == 2
    assert [r for r in caplog.records if "native-lm-batch" in r.getMessage() and "fan-out stub" in r.getMessage()]
