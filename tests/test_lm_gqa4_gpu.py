"""GPU: the native 5 Hz LM forward with FOUR q heads per kv head (Qwen3-4B's 32 / 8 layout, ``allow_gqa4=True``) against the oracle
composition (tests/_lm_oracle.py, configurations of tests/_lm_gqa4_oracle.py) and fixture G25.

The cases are tests/test_lm_gpu.py's, on the new layout: every parity gate is the project's rule (tests/_drift.py) - relative L2 per
sequence and over the whole tensor below 2 x the oracle's own bf16-storage drift, measured in the same run (or G25's, for the recorded
case).  A wrong q -> kv head map or a wrong pass of the decode kernel's LDS merge is an O(1) error against gates near 1.5e-2.
"""
import pytest
import torch

import _drift
import _lm_gqa4_oracle as Q
import _lm_oracle as L
import _lm_score_ref as S

pytestmark = pytest.mark.gpu

MAX_POS = 1100   # the longest decode run ends at 1030


@pytest.fixture(scope="module")
def lms(gpu_device):
    """(name, max_seqs) -> NativeCausalLM; built on first use, closed at the end of the module."""
    from ace355.lm import NativeCausalLM
    made = {}

    def get(name, max_seqs=4):
        if (name, max_seqs) not in made:
            lm = NativeCausalLM(Q.CONFIGS[name], gpu_device, max_positions=MAX_POS, max_seqs=max_seqs, allow_gqa4=True)
            lm.load_state_dict(dict(Q.weights(name)))
            made[(name, max_seqs)] = lm
        return made[(name, max_seqs)]

    yield get
    for lm in made.values():
        lm.close()


_REF = {}


def _reference(name, ids, first, cols):
    """(fp32 oracle, bf16-storage emulation) logits [N, len(cols), V] of one causal pass; computed once per case and shared."""
    key = (name, tuple(ids.flatten().tolist()), tuple(first), tuple(cols))
    if key not in _REF:
        cfg, w = Q.CONFIGS[name], Q.weights(name)
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
    V = Q.CONFIGS[name].vocab_size
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
@pytest.mark.parametrize("name", ["gqa4_tiny", "gqa4_wide"])
def test_prefill_parity(lms, name, P):
    """The query-block and key-tile edges of the 64-wide causal kernel, with a first visible key inside a tile (5), on a tile edge (64 at
    P = 65) and in the last column; two head pairs per kv head."""
    lm = lms(name)
    first = [min(f, P - 1) for f in (0, 5, P - 1)]
    ids, _ = _case(name, P, [P - f for f in first], 0, 2500 + P)
    ref, emu = _reference(name, ids, first, [P - 1])
    out = lm.prefill(ids.cuda(), L.mask_of(first, P).cuda())
    assert out.device.type == "cuda" and lm.length == P
    _gate(f"{name} prefill P = {P}, first = {first}", out.cpu(), ref[:, 0], emu[:, 0])


def test_prefill_and_decode_vs_g25(lms):
    """Against transformers itself (fp32, eager, its own cache), with the drift recorded when the fixture was made."""
    from ace355 import weightgen
    lm, w = lms("gqa4_wide"), Q.weights("gqa4_wide")
    z = Q.load_g25()
    assert abs(weightgen.checksum(w) - float(z["checksum"])) <= 1e-9 * float(z["checksum"])
    ids, first, P = torch.from_numpy(z["ids"]).long(), [int(v) for v in z["first"]], int(z["P"])
    out = _run(lm, ids, first, P)
    ref = torch.from_numpy(z["logits"])
    assert ref.shape[0] == 5
    for t in range(ref.shape[0]):
        for n in range(3):
            _drift.check(f"G25 step {t} sequence {n}", L.rel(out[n, t], ref[t, n]), float(z["drift"][t, n]))
        _drift.check(f"G25 step {t} whole tensor", L.rel(out[:, t], ref[t]), float(z["drift_all"][t]))


# ------------------------------------------------------------------ decode
# (name, P, last length, first): the runs cross the split boundary 64 | 65 inside the 64-key regime and the regime boundaries 256 | 257 and
# 1024 | 1025 of csrc/lm_plan.h, with first[n] inside the first chunk (5) and inside a later one
DECODE_RUNS = [("gqa4_tiny", 60, 70, (0, 5, 59)), ("gqa4_tiny", 250, 262, (0, 5, 200)), ("gqa4_tiny", 1020, 1030, (0, 300, 1019)),
               ("gqa4_wide", 250, 262, (0, 5, 200))]


def test_decode_runs_cross_every_regime_of_the_plan():
    from ace355 import native
    starts = [s for s in range(1, MAX_POS) if s == 1 or native.lm_decode_plan(s)["chunk"] != native.lm_decode_plan(s - 1)["chunk"]]
    assert starts == [1, 257, 1025]
    for b in starts[1:]:
        assert any(P < b <= end for _n, P, end, _f in DECODE_RUNS), f"no run crosses the regime boundary at {b}"
    assert any(native.lm_decode_plan(P + 1)["splits"] < native.lm_decode_plan(end)["splits"] and
               native.lm_decode_plan(P + 1)["chunk"] == native.lm_decode_plan(end)["chunk"] for _n, P, end, _f in DECODE_RUNS)


@pytest.mark.parametrize("name,P,end,first", DECODE_RUNS)
def test_decode_parity(lms, name, P, end, first):
    lm = lms(name)
    ids, first = _case(name, P, [P - f for f in first], end - P, 2600 + P)
    cols = list(range(P - 1, end))
    ref, emu = _reference(name, ids, first, cols)
    out = _run(lm, ids, first, P)
    assert lm.length == end
    for t, c in enumerate(cols):
        _gate(f"{name} length {c + 1} ({'prefill' if t == 0 else 'decode'})", out[:, t], ref[:, t], emu[:, t])


def test_cache_against_native_recompute(lms):
    """Decode step t against a native prefill of the same P + t columns: other kernels, so no equal bits, but the same gate."""
    lm = lms("gqa4_tiny")
    name, P, end, first = DECODE_RUNS[0]
    ids, first = _case(name, P, [P - f for f in first], end - P, 2600 + P)
    cols = list(range(P - 1, end))
    ref, emu = _reference(name, ids, first, cols)
    out = _run(lm, ids, first, P)
    for t in (1, 5, 10):
        again = lm.prefill(ids[:, :P + t], L.mask_of(first, P + t)).cpu()
        assert lm.length == P + t
        drift = L.rel(emu[:, t], ref[:, t])
        _drift.check(f"decode step {t} vs native prefill of {P + t} columns", L.rel(out[:, t], again), drift)
        _gate(f"native prefill of {P + t} columns", again, ref[:, t], emu[:, t])


def test_n16_decode_fills_the_z_grid(lms):
    """16 sequences (the handle's most) with 16 different first keys: one decode workgroup per (chunk, kv head, sequence)."""
    name, P, end = "gqa4_tiny", 20, 23
    lm = lms(name, max_seqs=16)
    first = [0, 19, 5, 1] + list(range(2, 14))
    ids, first = _case(name, P, [P - f for f in first], end - P, 2700)
    cols = list(range(P - 1, end))
    ref, emu = _reference(name, ids, first, cols)
    out = _run(lm, ids, first, P)
    for t, c in enumerate(cols):
        _gate(f"{name} N = 16 length {c + 1}", out[:, t], ref[:, t], emu[:, t])
    alone = _run(lm, ids[5:6], first[5:6], P)   # ... and a sequence of it alone has the bits it has among the sixteen
    assert torch.equal(_bits(alone[0]), _bits(out[5]))


# ------------------------------------------------------------------ what a sequence's bits depend on
def test_pads_are_invisible_and_sequences_independent(lms):
    lm = lms("gqa4_tiny")
    V, P = Q.GQA4_TINY.vocab_size, 70
    ids, first = _case("gqa4_tiny", P, (70, 40, 3), 3, 2577)
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
    for n in range(3):   # a sequence alone against the same sequence in the batch
        alone = _run(lm, ids[n:n + 1], first[n:n + 1], P)
        assert torch.equal(_bits(alone[0]), _bits(base[n])), n


def test_same_calls_same_bits(lms):
    lm = lms("gqa4_wide")
    ids, first = _case("gqa4_wide", 130, (130, 125, 1), 5, 2588)
    a = _run(lm, ids, first, 130)
    b = _run(lm, ids, first, 130)
    assert torch.equal(_bits(a), _bits(b))


def test_fan_out_then_decode_tokens_equals_separate_runs(lms, gpu_device):
    """One CFG pair fanned out to B = 3 songs, then device-side tokens: song b has the bits of a run of the pair alone on its tokens.
    P = 60 running to 66 crosses the decode attention's 64 | 65 chunk split."""
    name, B, P, k = "gqa4_tiny", 3, 60, 6
    lm = lms(name, max_seqs=16)
    V = Q.CONFIGS[name].vocab_size
    ids, first = L.left_padded([P, P - 2], P, V, 2590)
    am = L.mask_of(first, P)
    tok = torch.randint(0, V, (k, B), generator=torch.Generator().manual_seed(2591))
    want = []
    for b in range(B):
        lm.prefill(ids, am)
        want.append(torch.stack([lm.decode_tokens(tok[t, b:b + 1].to(gpu_device)).cpu() for t in range(k)]))   # [k, 2, V]
    assert not torch.equal(want[0], want[1])
    lm.prefill(ids, am)
    lm.fan_out([0] * B + [1] * B)
    assert lm.length == P
    for t in range(k):
        got = lm.decode_tokens(tok[t].to(gpu_device)).cpu()
        assert got.shape == (2 * B, V)
        for b in range(B):
            assert torch.equal(_bits(got[b]), _bits(want[b][t, 0])) and torch.equal(_bits(got[B + b]), _bits(want[b][t, 1])), (t, b)
    assert lm.length == P + k and lm.bad_tokens() == 0


# ------------------------------------------------------------------ score
def test_score_on_a_wide_handle(lms):
    """tests/test_lm_score_gpu.py's handle-path gates: the log-prob vector within 2 x the emulation's drift of it; a rank moves by at
    most the number of oracle logits within twice the emulation's largest logit error of the target's - exact wherever the fp32
    oracle's gap decides it.  N = 2, lengths (64, 41) left-padded to P = 64, start (40, 50)."""
    name, P, start = "gqa4_wide", 64, [40, 50]
    lm, cfg, w = lms(name), Q.CONFIGS[name], Q.weights(name)
    ids, first = L.left_padded((64, 41), P, cfg.vocab_size, 2540)
    lp, rank = lm.score(ids.cuda(), L.mask_of(first, P).cuda(), start=start)
    assert lp.is_cuda and lp.shape == (sum(P - s for s in start),) and rank.dtype == torch.int32
    lp, rank = lp.cpu(), rank.cpu()
    with torch.no_grad():
        ref = L.lm_logits_at(cfg, w, ids, first, range(P))
        emu = _drift.emulated(L.lm_logits_at, cfg, w, ids, first, range(P))
    rows = [(n, c) for n in range(2) for c in range(start[n], P)]
    lr = torch.stack([ref[n, c - 1] for n, c in rows])
    le = torch.stack([emu[n, c - 1] for n, c in rows])
    t = torch.stack([ids[n, c] for n, c in rows])
    o_lp, o_rank = S.token_stats(lr, t)
    e_lp, _e_rank = S.token_stats(le, t)
    tol = 2.0 * float((le - lr).abs().max())
    near = ((lr - lr[torch.arange(len(rows)), t][:, None]).abs() <= tol).sum(1) - 1
    assert torch.isfinite(lp).all() and bool((lp <= 0).all())
    _drift.check(f"{name} score log-prob", L.rel(lp, o_lp), L.rel(e_lp, o_lp))
    drank = (rank.long() - o_rank.long()).abs()
    print(f"    {name} score: ranks moved on {int((drank > 0).sum())} of {len(drank)} rows, {int((near == 0).sum())} rows decided by the "
          f"oracle's gap, logit tolerance {tol:.2e}")
    assert bool((drank <= near).all()), (drank.tolist(), near.tolist())


# ------------------------------------------------------------------ refusals
def test_other_layouts_stay_refused(gpu_device):
    from ace355.config import LmConfig
    from ace355.lm import NativeCausalLM
    base = Q.GQA4_TINY.__dict__
    for kw in (dict(num_attention_heads=4, num_key_value_heads=4), dict(num_attention_heads=16, num_key_value_heads=2), dict(head_dim=64)):
        with pytest.raises(NotImplementedError):
            NativeCausalLM(LmConfig(**{**base, **kw}), gpu_device, max_positions=16, allow_gqa4=True)
    with pytest.raises(NotImplementedError):   # 8 / 2 without the opt-in: refused as 32 / 8 is
        NativeCausalLM(Q.GQA4_TINY, gpu_device, max_positions=16)
