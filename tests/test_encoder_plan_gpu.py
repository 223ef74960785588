"""GPU: the encoder stack executes its pass plan (csrc/encoder_plan.h) on a workspace sized by the same header.  For each of the five handle
kinds, at the tiny configurations of test_encoder_lifecycle_gpu.py: a small call, a larger one that makes the workspace (and the rope
tables) grow, and the small one again - the first and the third give the same bits, which are a fresh handle's.  LM: the decode steps the
pass plan reports for a run carry ace355_lm_decode_plan's cut at each step's length, and the run passes test_lm_gpu.py's recompute
yardstick."""
import pytest
import torch

import _drift
import _lm_oracle as L
import test_encoder_lifecycle_gpu as lifecycle
import test_lm_gpu as lm_tests

pytestmark = pytest.mark.gpu


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _calls(what):
    """(small, large): two calls of one handle kind; the large one needs more rows, more V^T and, for cond / textenc, more rope rows."""
    if what == "cond":
        order = torch.tensor([0, 1, 1])
        def call(Ll, Tref, lens):
            tmask = (torch.arange(9)[None] < torch.tensor([9, 4])[:, None]).long()
            lmask = (torch.arange(Ll)[None] < torch.tensor(lens)[:, None]).long()
            return lambda o: o(_rnd(1, 2, 9, 64), tmask, _rnd(2, 2, Ll, 64), lmask, _rnd(3, 3, Tref, 64), order)[0]
        return call(70, 33, [70, 0]), call(600, 130, [600, 21])
    if what == "detok":
        return (lambda o: o(_rnd(4, 2, 7, 256))), (lambda o: o(_rnd(5, 3, 40, 256)))
    if what == "tok":
        return (lambda o: o.pool(_rnd(6, 2, 7 * 5, 64))), (lambda o: o.pool(_rnd(7, 3, 40 * 5, 64)))
    ids = lambda S, seed: torch.randint(0, 500, (2, S), generator=torch.Generator().manual_seed(seed))
    return (lambda o: o(ids(65, 8)).last_hidden_state), (lambda o: o(ids(600, 9)).last_hidden_state)


@pytest.mark.parametrize("what", ["cond", "detok", "tok", "textenc"])
def test_regrown_workspace_keeps_the_bits(gpu_device, what):
    k = lifecycle._kinds()[what]
    small, large = _calls(what)
    obj = k.make(gpu_device)
    fresh = k.make(gpu_device)
    try:
        obj.load_state_dict(k.weights)
        fresh.load_state_dict(k.weights)
        first = small(obj)
        big = large(obj)
        third = small(obj)
        assert bool(torch.isfinite(first.float()).all()) and bool(torch.isfinite(big.float()).all())
        assert torch.equal(_bits(first), _bits(third)), "the small call after the workspace grew"
        assert torch.equal(_bits(first), _bits(small(fresh))), "the small call on a fresh handle"
        assert torch.equal(_bits(big), _bits(large(fresh))), "the large call on a handle that has only seen it"
    finally:
        obj.close()
        fresh.close()


@pytest.fixture(scope="module")
def tiny_lm(gpu_device):
    from ace355.lm import NativeCausalLM
    made = []

    def make():
        lm = NativeCausalLM(L.TINY, gpu_device, max_positions=lm_tests.MAX_POS, max_seqs=4)
        lm.load_state_dict(L.weights("tiny"))
        made.append(lm)
        return lm

    yield make
    for lm in made:
        lm.close()


def test_lm_regrown_workspace_keeps_the_bits(tiny_lm):
    """Prefill + two decode steps at P = 17, then at P = 130 (more rows), then at P = 17 again; and on a fresh handle."""
    lm, fresh = tiny_lm(), tiny_lm()
    ids_s, first_s = lm_tests._case("tiny", 17, (17, 12, 1), 2, 91)
    ids_l, first_l = lm_tests._case("tiny", 130, (130, 125, 1), 2, 92)
    first = lm_tests._run(lm, ids_s, first_s, 17)
    big = lm_tests._run(lm, ids_l, first_l, 130)
    third = lm_tests._run(lm, ids_s, first_s, 17)
    assert torch.equal(_bits(first), _bits(third))
    assert torch.equal(_bits(first), _bits(lm_tests._run(fresh, ids_s, first_s, 17)))
    assert torch.equal(_bits(big), _bits(lm_tests._run(fresh, ids_l, first_l, 130)))


def test_lm_pass_plan_reports_the_decode_plan_of_every_step():
    """For every length a decode step of test_lm_gpu.py's runs reaches (they cross 256 | 257 and 1024 | 1025): what the handle would launch."""
    from ace355 import native
    c = L.TINY
    for name, P, end, _first in lm_tests.DECODE_RUNS:
        c = L.CONFIGS[name]
        for length in range(P + 1, end + 1):
            p = native.encoder_pass_plan(c.hidden_size, c.intermediate_size, c.num_attention_heads, c.num_key_value_heads, c.num_hidden_layers, 3, 1,
                                         causal=1, has_cache=1, pos0=length - 1, max_pos=lm_tests.MAX_POS, max_seqs=4, has_first=1)
            d = native.lm_decode_plan(length)
            dec = [s for s in p["steps"] if s["kind"] == "decode_attn"]
            assert len(dec) == c.num_hidden_layers and all((s["len"], s["chunk"], s["splits"]) == (length, d["chunk"], d["splits"]) for s in dec), length


def test_lm_run_against_native_recompute(tiny_lm):
    """test_lm_gpu.py's yardstick on the planned executor: decode step t against a native prefill of the same P + t columns, under the
    oracle emulation's drift of that column (the reference is shared with test_lm_gpu.py)."""
    lm = tiny_lm()
    name, P, end, first = lm_tests.DECODE_RUNS[0]
    ids, first = lm_tests._case(name, P, [P - f for f in first], end - P, 400 + P)
    cols = list(range(P - 1, end))
    ref, emu = lm_tests._reference(name, ids, first, cols)
    out = lm_tests._run(lm, ids, first, P)
    for t in (1, 5, 10):
        again = lm.prefill(ids[:, :P + t], L.mask_of(first, P + t)).cpu()
        _drift.check(f"decode step {t} vs native prefill of {P + t} columns", L.rel(out[:, t], again), L.rel(emu[:, t], ref[:, t]))
        lm_tests._gate(f"decode step {t}", out[:, t], ref[:, t], emu[:, t])
