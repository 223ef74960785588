"""GPU: the native 5 Hz LM forward (transformers' Qwen3ForCausalLM: prefill, KV-cached decode steps, last-position logits) against the
oracle composition (tests/_lm_oracle.py) and fixture G21.

Every parity gate is the project's rule (tests/_drift.py): relative L2 per sequence and over the whole tensor below 2 x the oracle's own
bf16-storage drift, measured in the same run (or G21's, for the recorded case).  The oracle has no cache: one causal pass over the whole
length gives the logits of every decode step (tests/test_lm_cpu.py pins that against per-prefix recomputes).
"""
import ctypes as C

import pytest
import torch

import _drift
import _lm_oracle as L

pytestmark = pytest.mark.gpu

MAX_POS = 1100   # the longest decode run ends at 1030


@pytest.fixture(scope="module")
def lms(gpu_device):
    """name -> (NativeCausalLM, weights); built on first use, closed at the end of the module."""
    from ace355.lm import NativeCausalLM
    made = {}

    def get(name):
        if name not in made:
            w = L.weights(name)
            lm = NativeCausalLM(L.CONFIGS[name], gpu_device, max_positions=MAX_POS, max_seqs=4)
            sd = dict(w)
            if L.CONFIGS[name].tie_word_embeddings:
                sd["lm_head.weight"] = w["model.embed_tokens.weight"]   # as a tied checkpoint's state_dict lists it: accepted and dropped
            lm.load_state_dict(sd)
            made[name] = (lm, w)
        return made[name]

    yield get
    for lm, _w in made.values():
        lm.close()


_REF = {}


def _reference(name, ids, first, cols):
    """(fp32 oracle, bf16-storage emulation) logits [N, len(cols), V] of one causal pass; computed once per case and shared."""
    key = (name, tuple(ids.flatten().tolist()), tuple(first), tuple(cols))
    if key not in _REF:
        cfg, w = L.CONFIGS[name], L.weights(name)
        with torch.no_grad():
            _REF[key] = (L.lm_logits_at(cfg, w, ids, first, cols), _drift.emulated(L.lm_logits_at, cfg, w, ids, first, cols))
    return _REF[key]


def _gate(what, out, ref, emu):
    """Per sequence and whole tensor: relative L2 < 2 x the emulation's drift (prints measured / drift)."""
    assert out.shape == ref.shape and out.dtype == torch.float32 and torch.isfinite(out).all()
    for n in range(ref.shape[0]):
        _drift.check(f"{what} sequence {n}", L.rel(out[n], ref[n]), L.rel(emu[n], ref[n]))
    _drift.check(f"{what} whole tensor", L.rel(out, ref), L.rel(emu, ref))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _case(name, P, lengths, extra, seed):
    """Left-padded prompts [N, P] + `extra` teacher-forced columns."""
    V = L.CONFIGS[name].vocab_size
    ids, first = L.left_padded(lengths, P, V, seed)
    tail = torch.randint(0, V, (len(lengths), extra), generator=torch.Generator().manual_seed(seed + 1000))
    return torch.cat([ids, tail], 1), first


def _run(lm, ids, first, P):
    """Native prefill over ids[:, :P] + teacher-forced decode steps: [N, steps + 1, V] on the CPU."""
    out = [lm.prefill(ids[:, :P], L.mask_of(first, P)).cpu()]
    for t in range(P, ids.shape[1]):
        out.append(lm.decode(ids[:, t]).cpu())
        assert lm.length == t + 1
    return torch.stack(out, 1)


# ------------------------------------------------------------------ prefill
@pytest.mark.parametrize("P", [1, 17, 64, 65, 130])
@pytest.mark.parametrize("name", ["tiny", "tiny_untied", "wide"])
def test_prefill_parity(lms, name, P):
    """The query-block and key-tile edges of the 64-wide causal kernel, with a first visible key inside a tile (5), on a tile edge (64 at
    P = 65) and in the last column."""
    lm, _w = lms(name)
    first = [min(f, P - 1) for f in (0, 5, P - 1)]
    ids, _ = _case(name, P, [P - f for f in first], 0, 300 + P)
    ref, emu = _reference(name, ids, first, [P - 1])
    out = lm.prefill(ids.cuda(), L.mask_of(first, P).cuda())
    assert out.device.type == "cuda" and lm.length == P
    _gate(f"{name} prefill P = {P}, first = {first}", out.cpu(), ref[:, 0], emu[:, 0])


def test_wide_prefill_and_decode_vs_g21(lms):
    """Against transformers itself (fp32, eager, its own cache), with the drift recorded when the fixture was made."""
    from ace355 import weightgen
    lm, w = lms("wide")
    z = L.load_g21()
    assert abs(weightgen.checksum(w) - float(z["wide_checksum"])) <= 1e-9 * float(z["wide_checksum"])
    ids, first, P = torch.from_numpy(z["wide_ids"]).long(), [int(v) for v in z["wide_first"]], int(z["wide_P"])
    out = _run(lm, ids, first, P)
    ref = torch.from_numpy(z["wide_logits"])
    for t in range(ref.shape[0]):
        for n in range(3):
            _drift.check(f"G21 wide step {t} sequence {n}", L.rel(out[n, t], ref[t, n]), float(z["wide_drift"][t, n]))
        _drift.check(f"G21 wide step {t} whole tensor", L.rel(out[:, t], ref[t]), float(z["wide_drift_all"][t]))


# ------------------------------------------------------------------ decode
# (name, P, last length, first): the runs cross the split boundary 64 | 65 inside the 64-key regime, the regime boundaries 256 | 257 and
# 1024 | 1025 of csrc/lm_plan.h (checked below through ace355_lm_decode_plan), with first[n] inside the first chunk (5) and inside a later one
DECODE_RUNS = [("tiny", 60, 70, (0, 5, 59)), ("tiny", 250, 262, (0, 5, 200)), ("tiny", 1020, 1030, (0, 300, 1019)),
               ("wide", 250, 262, (0, 5, 200))]


def test_decode_runs_cross_every_regime_of_the_plan():
    from ace355 import native
    starts = [s for s in range(1, MAX_POS) if s == 1 or native.lm_decode_plan(s)["chunk"] != native.lm_decode_plan(s - 1)["chunk"]]
    assert starts == [1, 257, 1025]
    for b in starts[1:]:
        assert any(P < b <= end for _n, P, end, _f in DECODE_RUNS), f"no run crosses the regime boundary at {b}"
    assert any(native.lm_decode_plan(P + 1)["splits"] < native.lm_decode_plan(end)["splits"] and
               native.lm_decode_plan(P + 1)["chunk"] == native.lm_decode_plan(end)["chunk"] for _n, P, end, _f in DECODE_RUNS)
    p = native.lm_decode_plan(262)
    assert 200 // p["chunk"] >= 1 and 5 // p["chunk"] == 0


@pytest.mark.parametrize("name,P,end,first", DECODE_RUNS)
def test_decode_parity(lms, name, P, end, first):
    lm, _w = lms(name)
    ids, first = _case(name, P, [P - f for f in first], end - P, 400 + P)
    cols = list(range(P - 1, end))
    ref, emu = _reference(name, ids, first, cols)
    out = _run(lm, ids, first, P)
    assert lm.length == end
    for t, c in enumerate(cols):
        _gate(f"{name} length {c + 1} ({'prefill' if t == 0 else 'decode'})", out[:, t], ref[:, t], emu[:, t])


def test_cache_against_native_recompute(lms):
    """Decode step t against a native prefill of the same P + t columns: other kernels, so no equal bits, but the same gate."""
    lm, _w = lms("tiny")
    name, P, end, first = DECODE_RUNS[0]
    ids, first = _case(name, P, [P - f for f in first], end - P, 400 + P)
    cols = list(range(P - 1, end))
    ref, emu = _reference(name, ids, first, cols)
    out = _run(lm, ids, first, P)
    for t in (1, 5, 10):
        again = lm.prefill(ids[:, :P + t], L.mask_of(first, P + t)).cpu()
        assert lm.length == P + t
        drift = L.rel(emu[:, t], ref[:, t])
        _drift.check(f"decode step {t} vs native prefill of {P + t} columns", L.rel(out[:, t], again), drift)
        _gate(f"native prefill of {P + t} columns", again, ref[:, t], emu[:, t])


# ------------------------------------------------------------------ what a sequence's bits depend on
def test_pads_are_invisible_and_sequences_independent(lms):
    lm, _w = lms("tiny")
    V, P = L.TINY.vocab_size, 70
    ids, first = _case("tiny", P, (70, 40, 3), 3, 77)
    base = _run(lm, ids, first, P)
    pads = ids.clone()
    pads[1, :30] = torch.randint(0, V, (30,), generator=torch.Generator().manual_seed(1))
    pads[2, :67] = torch.randint(0, V, (67,), generator=torch.Generator().manual_seed(2))
    assert torch.equal(_bits(_run(lm, pads, first, P)), _bits(base)), "ids below first[n] must not reach the logits"
    vis = ids.clone()
    vis[1, 30] = (vis[1, 30] + 1) % V
    c = _run(lm, vis, first, P)
    assert torch.equal(_bits(c[0]), _bits(base[0])) and torch.equal(_bits(c[2]), _bits(base[2]))
    assert all(not torch.equal(c[1, t], base[1, t]) for t in range(4)), "a visible id must change every step's logits"
    other = ids.clone()
    other[0] = torch.randint(0, V, (ids.shape[1],), generator=torch.Generator().manual_seed(3))
    d = _run(lm, other, first, P)
    assert torch.equal(_bits(d[1:]), _bits(base[1:])) and not torch.equal(d[0], base[0])


def test_same_calls_same_bits(lms):
    lm, _w = lms("wide")
    ids, first = _case("wide", 130, (130, 125, 1), 5, 88)
    a = _run(lm, ids, first, 130)
    b = _run(lm, ids, first, 130)
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ state and refusals
def _raw(lm):
    from ace355 import native
    p32 = C.POINTER(C.c_int32)

    def prefill(ids, first, out):
        i32, f32 = ids.to(torch.int32).contiguous(), torch.tensor(first, dtype=torch.int32)
        return lm._lib.ace355_lm_prefill(lm._h, C.cast(i32.data_ptr(), p32), C.cast(f32.data_ptr(), p32), ids.shape[0], ids.shape[1],
                                         native.ptr(out), native.current_stream_ptr())

    def decode(ids, out):
        i32 = ids.to(torch.int32).contiguous()
        return lm._lib.ace355_lm_decode(lm._h, C.cast(i32.data_ptr(), p32), native.ptr(out), native.current_stream_ptr())

    return prefill, decode, native.last_error


def test_state_and_refusals(gpu_device):
    from ace355.lm import NativeCausalLM
    V = L.TINY.vocab_size
    lm = NativeCausalLM(L.TINY, gpu_device, max_positions=8, max_seqs=2)
    lm.load_state_dict(L.weights("tiny"))
    prefill, decode, err = _raw(lm)
    out = torch.zeros(2, V, device="cuda")
    ids, first = L.left_padded((6, 2), 6, V, 9)
    nxt = torch.tensor([4, 5])
    assert lm.length == 0
    assert decode(nxt, out) == 1 and "no prefill" in err() and lm.length == 0          # decode before any prefill
    assert prefill(ids, first, out) == 0 and lm.length == 6
    good = out.cpu().clone()
    assert decode(nxt, out) == 0 and lm.length == 7
    good_step = out.cpu().clone()
    # each refused with nothing launched: the output buffer keeps its bits and the length stays
    marker = torch.full_like(out, 7.0)
    for what, call, text in [
            ("bad id", lambda o: decode(torch.tensor([4, V]), o), "outside"),
            ("negative id", lambda o: decode(torch.tensor([-1, 5]), o), "outside"),
            ("bad prefill id", lambda o: prefill(torch.where(ids == ids[0, 2], torch.tensor(V), ids), first, o), "outside"),
            ("first = P", lambda o: prefill(ids, [0, 6], o), "first[1]"),
            ("first < 0", lambda o: prefill(ids, [-1, 2], o), "first[0]"),
            ("N > max_seqs", lambda o: prefill(torch.cat([ids, ids[:1]]), first + [0], torch.zeros(3, V, device="cuda")), "max_seqs"),
            ("P > max_positions", lambda o: prefill(torch.zeros(2, 9, dtype=torch.long), [0, 0], o), "max_positions")]:
        o = marker.clone()
        assert call(o) == 1 and text in err(), (what, err())
        torch.cuda.synchronize()
        assert torch.equal(o, marker) and lm.length == 7, what
    # the generation goes on where it was: the same step from the same state gives the same bits as a fresh run
    assert decode(torch.tensor([8, 9]), out) == 0 and lm.length == 8
    step2 = out.cpu().clone()
    assert decode(nxt, out) == 1 and "full" in err() and lm.length == 8                # length == max_positions
    assert prefill(ids, first, out) == 0 and lm.length == 6                            # a prefill after a generation resets the length
    assert torch.equal(_bits(out), _bits(good))
    assert decode(nxt, out) == 0 and torch.equal(_bits(out), _bits(good_step))
    assert decode(torch.tensor([8, 9]), out) == 0 and torch.equal(_bits(out), _bits(step2))
    # the Python layer refuses the same things before the library sees them
    with pytest.raises(ValueError):
        lm.decode(nxt)
    with pytest.raises(ValueError):
        lm.prefill(torch.zeros(3, 4, dtype=torch.long))
    lm.close()


def test_unsupported_head_layout_refused(gpu_device):
    from ace355.config import LmConfig
    from ace355.lm import NativeCausalLM
    for kw in (dict(num_attention_heads=32, num_key_value_heads=8), dict(num_attention_heads=4, num_key_value_heads=4), dict(head_dim=64)):
        with pytest.raises(NotImplementedError):
            NativeCausalLM(LmConfig(**{**L.TINY.__dict__, **kw}), gpu_device, max_positions=16)


# ------------------------------------------------------------------ the seam
def test_call_as_forward_pass_greedy_tokens(lms):
    """NativeCausalLM.__call__ driven exactly as LLMHandler._forward_pass drives the model, for G21's CFG pair, feeding the recorded tokens:
    wherever the oracle's top-1 / top-2 gap exceeds 4 x the emulation's largest logit error, the native argmax is the oracle's."""
    lm, w = lms("tiny")
    z = L.load_g21()
    ids, first, P = torch.from_numpy(z["seam_ids"]).long().cuda(), [int(v) for v in z["seam_first"]], int(z["seam_P"])
    cols = list(range(P - 1, P + 7))
    ref, emu = _reference("tiny", ids.cpu()[:, :P + 7], first, cols)
    mask = L.mask_of(first, P).cuda()
    past, qualified = None, 0
    for t in range(8):
        if t == 0:
            o = lm(input_ids=ids[:, :P], attention_mask=mask, use_cache=True)
        else:
            mask = torch.cat([mask, torch.ones(2, 1, dtype=mask.dtype, device="cuda")], 1)
            o = lm(input_ids=ids[:, P + t - 1:P + t], past_key_values=past, attention_mask=mask, use_cache=True)
        past = o.past_key_values
        logits = o.logits[:, -1, :]
        assert o.logits.shape == (2, 1, L.TINY.vocab_size) and logits.dtype == torch.float32 and lm.length == P + t
        top2 = ref[:, t].topk(2, dim=-1).values
        gap, err = float((top2[:, 0] - top2[:, 1]).min()), float((emu[:, t] - ref[:, t]).abs().max())
        print(f"    step {t}: top-1 / top-2 gap {gap:.4f}, emulation's max logit error {err:.4f}, native's {float((logits.cpu() - ref[:, t]).abs().max()):.4f}")
        if gap > 4.0 * err:
            qualified += 1
            assert torch.equal(logits.argmax(-1).cpu(), ref[:, t].argmax(-1)), f"step {t}"
            assert torch.equal(ref[:, t].argmax(-1), ids.cpu()[:, P + t])
    assert qualified >= 6, f"only {qualified} of 8 steps qualify"


def test_seam_errors_before_any_launch(lms):
    lm, _w = lms("tiny")
    ids, first = _case("tiny", 20, (20, 11), 2, 55)
    ids = ids.cuda()
    mask = L.mask_of(first, 20).cuda()
    one = torch.ones(2, 1, dtype=mask.dtype, device="cuda")
    o0 = lm(input_ids=ids[:, :20], attention_mask=mask, use_cache=True)
    mask21 = torch.cat([mask, one], 1)
    o1 = lm(input_ids=ids[:, 20:21], past_key_values=o0.past_key_values, attention_mask=mask21, use_cache=True)
    good = dict(input_ids=ids[:, 21:22], past_key_values=o1.past_key_values, attention_mask=torch.cat([mask21, one], 1), use_cache=True)
    for what, kw in [("stale token", {**good, "past_key_values": o0.past_key_values}),
                     ("mask of the wrong width", {**good, "attention_mask": mask21}),
                     ("position_ids", {**good, "position_ids": torch.full((2, 1), 21, device="cuda")})]:
        with pytest.raises(NotImplementedError):
            lm(**kw)
        assert lm.length == 21, what
    o2 = lm(**good)   # the refused calls changed nothing: the generation goes on, as in an undisturbed run
    lm.prefill(ids[:, :20], mask)
    lm.decode(ids[:, 20])
    assert torch.equal(_bits(lm.decode(ids[:, 21])), _bits(o2.logits[:, 0]))


class _Stub(torch.nn.Module):
    """The kept PyTorch module of the swap: records its calls and returns a cache object of its own."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, **kw):
        self.calls.append(past_key_values)
        cache = past_key_values if past_key_values is not None else ["stub-cache"]
        return type("Out", (), {"logits": torch.zeros(input_ids.shape[0], 1, 4), "past_key_values": cache})()


def test_swap_routes_to_native_or_kept_module(lms):
    from ace355.modswap import NativeCausalLMSwap
    lm, _w = lms("tiny")
    stub = _Stub()
    sw = NativeCausalLMSwap(lm, stub, "llm")
    ids, first = _case("tiny", 20, (20, 11), 1, 56)
    mask, one = L.mask_of(first, 20), torch.ones(2, 1, dtype=torch.long)
    o = sw(input_ids=ids[:, :20], attention_mask=mask, use_cache=True)
    o = sw(input_ids=ids[:, 20:21], past_key_values=o.past_key_values, attention_mask=torch.cat([mask, one], 1), use_cache=True)
    assert stub.calls == [] and sw.native_calls == 2 and o.logits.shape == (2, 1, L.TINY.vocab_size) and lm.length == 21
    holes = mask.clone()
    holes[0, 3] = 0
    r = sw(input_ids=ids[:, :20], attention_mask=holes, use_cache=True)
    r2 = sw(input_ids=ids[:, 20:21], past_key_values=r.past_key_values, attention_mask=torch.cat([holes, one], 1), use_cache=True)
    assert stub.calls == [None, ["stub-cache"]] and r2.past_key_values is r.past_key_values and sw.native_calls == 2
    assert lm.length == 21, "the kept module's generation must not touch the native cache"
