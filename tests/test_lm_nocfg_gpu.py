"""GPU: the 5 Hz LM's non-CFG path - the logits stage in the model's dtype (``ace355_lm_shape_as``) bit for bit against its numpy
restatement (tests/_lm_nocfg_oracle.py, itself held to the reference's output by G26), the selection on bf16-valued rows full of ties,
the native non-CFG loop against the restated reference loop (tests/_lm_nocfg_ref.py) driven with the native forward, the bits of a
shared-prompt batch, ``generate_codes_batch_nocfg`` against the sequential loop per seed, and the ``_run_pt`` seam."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

import _lm_batch_ref as S
import _lm_logits_oracle as O
import _lm_loop_ref as R
import _lm_nocfg_oracle as N
import _lm_nocfg_ref as NR
import _lm_oracle as L
import _lm_sample_oracle as SO

pytestmark = pytest.mark.gpu

REAL_V = 217205
V_TINY = L.TINY.vocab_size
TOP_P, TEMP = 0.9, 0.85
SEEDS = [101, 202, 303, 404, 505, 606, 707, 808, 909, 1010, 1111, 1212, 1313, 1414, 1515, 1616]
HALF_06 = (0.62109375, -0.62109375, 11.8125, -11.8125)   # bf16 values whose fp32 quotient by 0.6 is a tie between two bf16 neighbours


# ------------------------------------------------------------------ the stage
def _inputs(B, V, seed):
    """logits [B, V]: fp32 ``randn * 3`` (not bf16 values: the stage's first rounding is the model's cast) with -inf, signed zeros, a
    NaN, fp32 values that are ties between two bf16 neighbours, values past bf16's range and subnormals planted; a codes mask, an
    "understand" mask, eos, history."""
    g = torch.Generator().manual_seed(seed)
    cond = (torch.randn(B, V, generator=g) * 3).numpy()
    rng = np.random.default_rng(seed)
    cond[rng.random((B, V)) < 0.02] = -np.inf
    cond[rng.random((B, V)) < 0.02] = -0.0
    cond[rng.random((B, V)) < 0.01] = 0.0
    special = np.array([1.00390625, 1.01171875, -1.00390625, 3.4e38, -3.4e38, 1e-40, -4.6e-41, np.nan, np.inf] + list(HALF_06), dtype=np.float32)
    pos = rng.integers(0, V, size=(B, len(special)))
    for b in range(B):
        cond[b, pos[b]] = special[:len(pos[b])]
    eos = V - 1 if V < 3 else V - 3
    mask = np.where(rng.random(V) < 0.5, 0.0, -np.inf).astype(np.float32)
    mask[eos] = 0.0
    amask = np.where(mask == 0, -np.inf, 0.0).astype(np.float32)
    hist = rng.integers(-2, V + 2, size=(B, 40))
    hist[:, 1] = hist[:, 0]
    hist[:, 2:2 + min(6, pos.shape[1])] = pos[:, :6]              # some of the planted values meet the penalty
    return cond, mask, amask, eos, hist


def _settings():
    """Every processor branch of G26 (a) with the temperatures and penalties cycling through them."""
    temps, pens = (None, 0.7, 0.6, 0.0), (1.0, 1.1, 1.3)
    return [(m, temps[(i + j) % 4], pens[(2 * i + j) % 3]) for i, m in enumerate(O.MODE_NAMES) for j in range(2)]


def _bits_equal(got, want: np.ndarray, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    if not O.same_bits(got, want):
        bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        r, v = bad[0]
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at row {r} id {v}: {got[r, v]!r} vs {want[r, v]!r}")


def _native(dev, cond, mask, amask, eos, hist, mode, T, pen, layout="dense", dtype=torch.bfloat16):
    from ace355.lmlogits import SeenTokens, shape_logits
    B, V = cond.shape
    which, eos_mode = O.MODES[mode]
    m = {"codes": mask, "audio": amask, None: None}[which]

    def put(a):
        if layout != "strided":
            return torch.from_numpy(a).to(dev)
        wide = torch.full((B, V + 13), 7.0, device=dev)          # rows strided out of a wider tensor, base off 16 bytes
        wide[:, 5:5 + V] = torch.from_numpy(a).to(dev)
        return wide[:, 5:5 + V]
    c = put(cond)
    seen = SeenTokens(B, V, dev).mark(torch.from_numpy(hist).to(dev)) if pen != 1.0 else None
    out = c if layout == "alias" else (put(np.zeros_like(cond)) if layout == "strided" else None)
    got = shape_logits(c, None, 1.0, torch.from_numpy(m).to(dev) if m is not None else None, eos if eos_mode else None, eos_mode, T, pen,
                       seen, out=out, dtype=dtype)
    if layout == "alias":
        assert got.data_ptr() == c.data_ptr()
    return got


def _want(cond, mask, amask, eos, hist, mode, T, pen):
    which, eos_mode = O.MODES[mode]
    m = {"codes": mask, "audio": amask, None: None}[which]
    return N.shape(cond, m, eos, eos_mode, T, pen, O.seen_bitmap(hist, cond.shape[1]))


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 8191, 8192, 8193, 2 * 8192 + 1])
def test_shape_bf16_equals_the_oracle_bit_for_bit(gpu_device, V, B):
    """Chunk edges of plan_lm_pick (8192), head / tail of the 16-byte groups (odd V: every row has another alignment), every branch."""
    a = _inputs(B, V, 100 * V + B)
    for i, (mode, T, pen) in enumerate(_settings()):
        layout = ("dense", "strided", "alias")[i % 3]
        want = _want(*a, mode, T, pen)
        assert N.is_bf16(want)
        _bits_equal(_native(gpu_device, *a, mode, T, pen, layout), want, (V, B, mode, T, pen, layout))


def test_shape_bf16_divides_the_halfway_quotients_and_differs_from_fp32(gpu_device):
    """The inputs do hold what the roundings are about: quotients by 0.6 that are bf16 ties, and results the fp32 stage gives otherwise."""
    a = _inputs(3, 8193, 26)
    pre = _want(*a, "none", None, 1.0)
    assert int(N.halfway_mask(pre, 0.6).sum()) >= 3
    got = _native(gpu_device, *a, "none", 0.6, 1.3)
    _bits_equal(got, _want(*a, "none", 0.6, 1.3), "T 0.6")
    f32 = _native(gpu_device, *a, "none", 0.6, 1.3, dtype=torch.float32).cpu().numpy()
    assert not O.same_bits(got.cpu().numpy(), f32)


def test_shape_bf16_strided_rows_leave_the_gaps_alone(gpu_device):
    from ace355.lmlogits import shape_logits
    B, V = 3, 8193
    cond, mask, _am, eos, _h = _inputs(B, V, 7)
    wide = torch.full((B, V + 11), float("nan"), device=gpu_device)
    out = wide[:, 3:3 + V]
    shape_logits(torch.from_numpy(cond).to(gpu_device), None, 1.0, torch.from_numpy(mask).to(gpu_device), eos, O.EOS_BLOCK, 0.7, out=out,
                 dtype=torch.bfloat16)
    _bits_equal(out, N.shape(cond, mask, eos, O.EOS_BLOCK, 0.7), "strided out")
    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + V:]).all()


def test_shape_bf16_row_does_not_depend_on_batch_or_neighbours(gpu_device):
    B, V = 16, 8193
    a = _inputs(B, V, 11)
    cond, mask, amask, eos, hist = a
    full = _native(gpu_device, *a, "block", 0.6, 1.3).cpu().numpy()
    for r in (0, 5, 15):
        alone = _native(gpu_device, cond[r:r + 1], mask, amask, eos, hist[r:r + 1], "block", 0.6, 1.3)
        _bits_equal(alone, full[r:r + 1], f"row {r} alone")
    c2, h2 = np.full_like(cond, np.nan), np.zeros_like(hist)
    c2[5], h2[5] = cond[5], hist[5]
    _bits_equal(_native(gpu_device, c2, mask, amask, eos, h2, "block", 0.6, 1.3)[5:6], full[5:6], "row 5 among NaN rows")


def test_shape_bf16_at_the_real_vocabulary(gpu_device):
    a = _inputs(2, REAL_V, 2051)
    for mode, T, pen, layout in (("block", 0.6, 1.3, "dense"), ("force", None, 1.1, "alias"), ("understand", 0.0, 1.0, "strided")):
        _bits_equal(_native(gpu_device, *a, mode, T, pen, layout), _want(*a, mode, T, pen), (mode, T, pen, layout))


def _raw_shape_as(dev, cond, uncond, out, p, dtype):
    from ace355 import native
    with torch.cuda.device(dev):
        return native.lib().ace355_lm_shape_as(cond.data_ptr(), cond.stride(0), uncond.data_ptr() if uncond is not None else None,
                                               uncond.stride(0) if uncond is not None else 0, out.data_ptr(), out.stride(0),
                                               cond.shape[0], cond.shape[1], C.byref(p), dtype, native.current_stream_ptr())


def test_shape_as_f32_is_bit_equal_to_shape(gpu_device):
    """``ace355_lm_shape_as(ACE355_DTYPE_F32)`` and ``ace355_lm_shape`` on the same inputs, with and without the CFG pair."""
    from ace355 import native
    from ace355.lmlogits import SeenTokens, shape_logits
    for B, V in ((3, 8193), (16, 33), (2, 2 * 8192 + 1)):
        cond, mask, _am, eos, hist = _inputs(B, V, 300 + V)
        g = torch.Generator().manual_seed(V)
        c, u = torch.from_numpy(cond).to(gpu_device), (torch.randn(B, V, generator=g) * 3).to(gpu_device)
        m = torch.from_numpy(mask).to(gpu_device)
        seen = SeenTokens(B, V, gpu_device).mark(torch.from_numpy(hist).to(gpu_device))
        for uncond in (u, None):
            for T, pen, mode in ((0.6, 1.3, O.EOS_BLOCK), (None, 1.0, O.EOS_FORCE), (0.7, 1.1, O.EOS_NONE)):
                want = shape_logits(c, uncond, 1.7, m, eos if mode else None, mode, T, pen, seen)
                p = native.LmShapeParamsC(cfg_scale=1.7, eos_id=eos if mode else -1, eos_mode=mode, has_temperature=0 if T is None else 1,
                                          temperature=T or 0.0, penalty=pen, mask=m.data_ptr(), seen=seen.words.data_ptr() if pen != 1.0 else None)
                out = torch.empty_like(c)
                assert _raw_shape_as(gpu_device, c, uncond, out, p, native.DTYPE_F32) == 0, native.last_error()
                _bits_equal(out, want.cpu().numpy(), (B, V, uncond is not None, T, pen, mode))


def test_shape_as_refusals_happen_before_a_launch(gpu_device):
    """With real device memory: each refusal returns ACE355_ERR_INVALID and ``out`` keeps its bytes."""
    from ace355 import native
    B, V = 2, 100
    c = torch.randn(B, V, device=gpu_device)
    out = torch.full((B, V), 7.0, device=gpu_device)
    seen = torch.zeros(B, 4, dtype=torch.int32, device=gpu_device)
    base = dict(cfg_scale=2.0, eos_id=5, eos_mode=1, has_temperature=1, temperature=0.85, penalty=1.1, mask=None, seen=seen.data_ptr())
    bad = [(dict(), 2, None, "dtype must"), (dict(), -1, None, "dtype must"), (dict(), native.DTYPE_BF16, c, "fp32 only"),
           (dict(eos_id=V), native.DTYPE_BF16, None, "eos_id"), (dict(eos_mode=3), native.DTYPE_BF16, None, "eos_mode"),
           (dict(penalty=0.0), native.DTYPE_BF16, None, "penalty"), (dict(seen=None), native.DTYPE_BF16, None, "seen"),
           (dict(temperature=0.0), native.DTYPE_BF16, None, "temperature"), (dict(cfg_scale=float("nan")), native.DTYPE_F32, c, "cfg_scale")]
    for change, dtype, uncond, word in bad:
        p = native.LmShapeParamsC(**{**base, **change})
        assert _raw_shape_as(gpu_device, c, uncond, out, p, dtype) == 1 and "lm_shape_as:" in native.last_error() and word in native.last_error()
    p = native.LmShapeParamsC(**base)
    lib = native.lib()
    for cs, os_, B_, V_, word in ((V - 1, V, B, V, "stride"), (V, V - 1, B, V, "stride"), (V, V, 0, V, "B must"), (V, V, B, 0, "V must")):
        assert lib.ace355_lm_shape_as(c.data_ptr(), cs, None, 0, out.data_ptr(), os_, B_, V_, C.byref(p), native.DTYPE_BF16, None) == 1
        assert "lm_shape_as:" in native.last_error() and word in native.last_error()
    torch.cuda.synchronize(gpu_device)
    assert bool((out == 7.0).all())
    assert _raw_shape_as(gpu_device, c, None, out, p, native.DTYPE_BF16) == 0     # and the same call without a defect runs
    torch.cuda.synchronize(gpu_device)
    assert not bool((out == 7.0).any())
    from ace355.lmlogits import shape_logits
    with pytest.raises(ValueError):
        shape_logits(c, dtype=torch.float16)
    with pytest.raises(ValueError):
        shape_logits(c, c, dtype=torch.bfloat16)


# ------------------------------------------------------------------ the selection on rows full of ties
MARGIN = 1e-4
PICK_SETTINGS = [(None, 0.9), (50, None), (None, None)]


def _tied_rows(V, B, seed):
    """[B, V] bf16-valued fp32 rows: ``randn * 3`` rounded to bf16 and twelve planted peaks in three tie groups, so that the nucleus
    cut falls inside or beside a group of equal values; each row re-drawn until its top-p walk keeps the margin (as
    tests/test_lm_sample_gpu.py does: both sides sum in fp64 and differ by rounding of the sums only)."""
    rows, s = [], seed * 1000
    while len(rows) < B:
        s += 1
        g = np.random.default_rng(s)
        x = N.rne((g.standard_normal(V) * 3).astype(np.float32))
        x[g.choice(V, 12, replace=False)] = np.repeat(np.array([22.0, 21.5, 21.0], dtype=np.float32), 4)
        if all(SO.top_p_margin(x, k, p)[0] >= MARGIN for k, p in PICK_SETTINGS):
            rows.append(x)
    return np.stack(rows)


def test_pick_on_bf16_valued_rows_with_ties_equals_the_oracle(gpu_device):
    from ace355 import lmsample
    V, B = 8193, 3
    xnp = _tied_rows(V, B, 26)
    assert N.is_bf16(xnp)
    for r in range(B):
        _vals, counts = np.unique(xnp[r], return_counts=True)
        assert counts[counts > 1].sum() >= V / 10                # at least a tenth of the entries share their value with another
    x = torch.from_numpy(xnp).to(gpu_device)
    inside = 0
    for k, p in PICK_SETTINGS:
        masks = [SO.keep_mask(xnp[r], k, p) for r in range(B)]
        tok, kept, keep = lmsample.pick(x, k, p, 0.0, None, want_kept=True, want_mask=True)
        tok, kept, keep = tok.cpu().numpy(), kept.cpu().numpy(), keep.cpu().numpy().astype(bool)
        for r in range(B):
            assert np.array_equal(keep[r], masks[r]), (r, k, p, int(keep[r].sum()), int(masks[r].sum()))
            assert kept[r] == masks[r].sum() and tok[r] == SO.greedy_token(xnp[r], masks[r]), (r, k, p)
            if p is not None:                                    # the cut falls between two equal values
                inside += int(not SO.top_p_margin(xnp[r], k, p)[1])
        u = np.array([0.05, 0.5, 0.93], dtype=np.float32)
        tok2, kept2, keep2 = lmsample.pick(x, k, p, TEMP, torch.from_numpy(u).to(gpu_device), want_kept=True, want_mask=True)
        assert np.array_equal(keep2.cpu().numpy().astype(bool), keep) and np.array_equal(kept2.cpu().numpy(), kept)
        for r in range(B):
            assert tok2[r].item() == SO.token_for_u(xnp[r], masks[r], TEMP, u[r]), (r, k, p)
    assert inside >= 1, "no row's nucleus cut fell inside a tie group: the inputs do not test what they are for"


# ------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def lms(gpu_device):
    from ace355.lm import NativeCausalLM
    out = {}
    for name, dtype in NR.DTYPES.items():
        out[name] = NativeCausalLM(L.TINY, gpu_device, max_positions=72, max_seqs=16, out_dtype=dtype)
        out[name].load_state_dict(dict(L.weights("tiny")))
    yield out
    for lm in out.values():
        lm.close()


class _Streamer:
    def __init__(self):
        self.put_calls, self.ended = [], 0

    def put(self, t):
        self.put_calls.append(t.cpu())

    def end(self):
        self.ended += 1


class _RefBase:
    def _build_logits_processor(self, repetition_penalty):
        if repetition_penalty == 1.0:
            return []
        return [lambda ids, scores: R.repetition_penalty(ids, scores, repetition_penalty)]

    def _generate_with_constrained_decoding(self, *a, **k):
        raise AssertionError("the reference's loop must not be asked")


def _handler(lm, gpu_device):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _RefBase):
        pass

    h = Handler()
    h.llm, h.device, h.use_native_lm_nocfg = lm, gpu_device, True
    h.llm_tokenizer = R.FakeTokenizer(R.EOS)
    return h


def _processor(phase, target, T):
    if phase == "target":
        return R.make_processor(target, T)
    return NR.make_processor(phase, T)


def _both(lm, gpu_device, B, phase, target, pair, max_new, streamer=False, seed=5):
    """(native ids, stats, processor, streamer), (yardstick ids, processor, streamer) for the same prompt, settings and torch seed.
    The yardstick is the restated loop on ``lm.prefill`` / ``lm.decode``; its stage is the reference's torch operations in the
    model's dtype on the CPU (that defines the bits), its selection ``select_tokens`` on the result moved back as fp32."""
    from ace355 import lmsample
    pen, T = (2.0, 0.5) if pair else (1.0, None)
    ids, am = NR.loop_prompt(B)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    h = _handler(lm, gpu_device)
    p1, s1 = _processor(phase, target, T), _Streamer() if streamer else None
    torch.manual_seed(seed)
    got = h._generate_with_constrained_decoding(ids, am, max_new, TEMP, None, TOP_P, pen, R.PAD, s1, p1)
    p2, s2 = _processor(phase, target, T), _Streamer() if streamer else None
    cpu_stage = NR.torch_stage(lm.out_dtype, pen)
    torch.manual_seed(seed)
    with torch.inference_mode():
        want = NR.run_loop(lambda g, step: lm.prefill(g, am) if step == 0 else lm.decode(g[:, -1]),
                           lambda logits, cur, p: cpu_stage(logits.cpu(), cur.cpu(), p).float().to(gpu_device),
                           lambda x: lmsample.select_tokens(x, None, TOP_P, TEMP), ids, max_new, R.EOS, R.PAD, p2, s2)
    return (got, h._lm_loop_stats, p1, s1), (want, p2, s2)


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "penalty2_T0.5"])
@pytest.mark.parametrize("target", [6, 10])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dt", list(NR.DTYPES))
def test_loop_with_a_target_matches_and_reads_two_tokens(lms, gpu_device, dt, B, target, pair):
    (got, stats, p1, _s), (want, p2, _s2) = _both(lms[dt], gpu_device, B, "target", target, pair, 14)
    assert got.dtype == want.dtype and got.device == want.device and torch.equal(got, want)
    steps = -(-target // B) + 1
    assert got.shape == (B, 6 + steps) and (got[:, -1] == R.EOS).all() and ((got[:, 6:-1] >= 300) & (got[:, 6:-1] < 900)).all()
    assert p1.state == p2.state == R.FSMState.CODES_GENERATION and p1.codes_count == p2.codes_count == B * steps
    assert stats["cfg"] is False and stats["steps"] == steps and stats["native_steps"] == steps - 1
    assert stats["token_reads"] <= 2 and stats["sync_free_steps"] == stats["native_steps"] - 1


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "penalty2_T0.5"])
@pytest.mark.parametrize("phase", ["understand", "none", "disabled", "free"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dt", list(NR.DTYPES))
def test_free_phases_match_and_read_every_step(lms, gpu_device, dt, B, phase, pair):
    """"understand": ``COMPLETED`` with the ``audio_code_mask``, the free-form text; no processor; a disabled one; codes without a
    target.  Nothing blocks EOS there, so every step reads its tokens; the streamer sees every step's tokens."""
    (got, stats, p1, s1), (want, p2, s2) = _both(lms[dt], gpu_device, B, phase, None, pair, 8, streamer=phase == "understand")
    assert got.dtype == want.dtype and torch.equal(got, want)
    steps = got.shape[1] - 6
    assert 1 <= steps <= 8 and stats["cfg"] is False
    assert stats["sync_free_steps"] == 0 and stats["token_reads"] == stats["steps"] == steps
    assert stats["native_steps"] == (steps - 1 if phase == "free" else steps)
    if p1 is not None:
        assert p1.state == p2.state and p1.codes_count == p2.codes_count
    if phase == "understand":
        assert not ((got[:, 6:] >= 300) & (got[:, 6:] < 900)).any() and p1.state == R.FSMState.COMPLETED
        assert s1.ended == s2.ended == 1 and len(s1.put_calls) == len(s2.put_calls) == steps
        assert all(torch.equal(a, b) and a.shape == (B, 1) for a, b in zip(s1.put_calls, s2.put_calls))
    stopped = ((got[:, -1] == R.EOS) | (got[:, -1] == R.PAD)).any().item()
    assert stopped or steps == 8                                 # the stop rule: any row on EOS or pad, else max_new_tokens


class _NanLm:
    """What generate_constrained asks of a NativeCausalLM, with logits that turn NaN at one step."""
    out_dtype, cfg, max_seqs = torch.bfloat16, L.TINY, 16

    def __init__(self, dev, nan_step):
        self.dev, self.nan_step, self.step, self.fed = dev, nan_step, 0, []

    def _logits(self, rows):
        x = torch.randn(rows, V_TINY, device=self.dev)
        if self.step == self.nan_step:
            x[0, 400] = float("nan")
        self.step += 1
        return x

    def prefill(self, ids, mask):
        return self._logits(ids.shape[0])

    def decode_tokens(self, tokens):
        self.fed.append(tokens.clone())
        return self._logits(tokens.shape[0])

    def bad_tokens(self):
        return 0


@pytest.mark.parametrize("sync_free", [False, True])
def test_loop_raises_when_a_step_could_draw_no_token(gpu_device, sync_free):
    from ace355.lmlogits import generate_constrained
    ids, am = NR.loop_prompt(2)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    h = _RefBase()
    h.llm_tokenizer = R.FakeTokenizer(R.EOS)
    stub = _NanLm(gpu_device, nan_step=2)
    proc = R.make_processor(40, None) if sync_free else None
    torch.manual_seed(1)
    with pytest.raises(RuntimeError, match="no valid token"):
        generate_constrained(h, stub, ids, am, 6, TEMP, None, TOP_P, 1.0, R.PAD, None, proc)
    if sync_free:
        assert h._lm_loop_stats["steps"] == 6 and h._lm_loop_stats["token_reads"] == 1 and proc.codes_count == 12
        assert stub.fed[2][0].item() == -1 and (stub.fed[2][1] >= 300).item()
    else:
        assert h._lm_loop_stats["steps"] == 3 and len(stub.fed) == 2


# ------------------------------------------------------------------ the bits of a shared-prompt batch
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("B", [2, 3, 16])
@pytest.mark.parametrize("dt", list(NR.DTYPES))
def test_every_row_of_a_shared_prompt_batch_has_the_single_sequence_bits(lms, gpu_device, dt, B):
    """After ``prefill([1, P])``, ``fan_out([0] * B)`` and ``decode_tokens``, every row's logits are bit-equal to the N = 1 sequence's
    decode of the same token: why song i of the batched loop can equal the loop run alone."""
    lm = lms[dt]
    ids, am = NR.loop_prompt(1)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    toks = torch.randint(0, V_TINY, (3, B), generator=torch.Generator().manual_seed(B))
    toks[:, B - 1] = toks[:, 0]
    alone = {}
    for b in sorted({0, 1, B - 1}):                              # the N = 1 runs of three of the songs
        first = lm.prefill(ids, am).clone()
        alone[b] = [lm.decode_tokens(toks[t, b:b + 1].to(gpu_device)).clone() for t in range(3)]
    again = lm.prefill(ids, am).clone()
    assert torch.equal(_bits(again), _bits(first))
    lm.fan_out([0] * B)
    for t in range(3):
        got = lm.decode_tokens(toks[t].to(gpu_device))
        assert got.shape == (B, V_TINY)
        for b, rows in alone.items():
            assert torch.equal(_bits(got[b]), _bits(rows[t][0])), (t, b)
        assert torch.equal(_bits(got[B - 1]), _bits(got[0]))
    assert lm.bad_tokens() == 0


# ------------------------------------------------------------------ B songs, one loop
_SEQUENTIAL = {}


def _sequential_row(lm, gpu_device, seed, target, pair, temperature=TEMP):
    """The row of the B = 1 native non-CFG loop after ``torch.manual_seed(seed)`` with a fresh processor: computed once per case."""
    key = (lm.out_dtype, seed if temperature > 0 else None, target, pair, temperature)
    if key not in _SEQUENTIAL:
        pen, T = (2.0, 0.5) if pair else (1.0, None)
        ids, am = NR.loop_prompt(1)
        h, proc = _handler(lm, gpu_device), R.make_processor(target, T)
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        out = h._generate_with_constrained_decoding(ids.to(gpu_device), am.to(gpu_device), target + 10, temperature, None, TOP_P, pen, R.PAD,
                                                    None, proc)
        assert proc.codes_count == target + 1 and h._lm_loop_stats["steps"] == target + 1
        _SEQUENTIAL[key] = out[0].cpu()
    return _SEQUENTIAL[key]


def _batched(lm, gpu_device, seeds, target, pair, temperature=TEMP):
    from ace355.lmlogits import generate_codes_batch_nocfg
    pen, T = (2.0, 0.5) if pair else (1.0, None)
    ids, am = NR.loop_prompt(1)
    h, proc = _handler(lm, gpu_device), R.make_processor(target, T)
    out = generate_codes_batch_nocfg(h, lm, ids.to(gpu_device), am.to(gpu_device), seeds, target + 10, temperature, None, TOP_P, pen, R.PAD, proc)
    return out, h._lm_loop_stats, proc


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "penalty2_T0.5"])
@pytest.mark.parametrize("B", [2, 3, 16])
@pytest.mark.parametrize("dt", list(NR.DTYPES))
def test_every_song_equals_the_sequential_loop_for_its_seed(lms, gpu_device, dt, B, pair):
    lm, target = lms[dt], 6
    seeds = SEEDS[:B]
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(gpu_device)
    got, stats, proc = _batched(lm, gpu_device, seeds, target, pair)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(gpu_device), gpu_state)
    assert lm.length == 6 + target and len(lm._first) == B
    want = torch.stack([_sequential_row(lm, gpu_device, s, target, pair) for s in seeds])
    assert got.dtype == torch.int64 and got.device == gpu_device and got.shape == (B, 6 + target + 1)
    assert torch.equal(got.cpu(), want)
    assert (got[:, -1] == R.EOS).all() and ((got[:, 6:-1] >= 300) & (got[:, 6:-1] < 900)).all()
    assert len({tuple(r.tolist()) for r in got.cpu()}) > 1       # the seeds do steer the songs
    assert stats["steps"] == target + 1 and stats["token_reads"] <= 2 and stats["batch"] == B and stats["prefill_rows"] == 1
    assert stats["native_steps"] == target and stats["sync_free_steps"] == target - 1 and stats["cfg"] is False
    assert proc.codes_count == target + 1 and proc.state == R.FSMState.CODES_GENERATION


def test_equal_seeds_give_equal_songs_and_greedy_gives_one_song(lms, gpu_device):
    lm = lms["bf16"]
    got, _stats, _proc = _batched(lm, gpu_device, [707, 202, 707], 6, True)
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])
    assert torch.equal(got[1].cpu(), _sequential_row(lm, gpu_device, 202, 6, True))
    got, stats, proc = _batched(lm, gpu_device, [1, 2, 3, 4], 6, True, temperature=0.0)
    assert all(torch.equal(got[0], r) for r in got[1:])
    assert torch.equal(got[0].cpu(), _sequential_row(lm, gpu_device, 1, 6, True, temperature=0.0))
    assert stats["steps"] == 7 and proc.codes_count == 7


# ------------------------------------------------------------------ the seam
class NoCfgHost(S.StubHost):
    """``StubHost`` with the non-CFG branch of ``_run_pt_single`` (llm_inference.py:929-942): one row, ``padding=False``.  The host's
    own loop is a stand-in that appends one EOS and counts its calls."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.host_loops = 0

    def _generate_with_constrained_decoding(self, input_ids, attention_mask, max_new_tokens, temperature, top_k, top_p,
                                            repetition_penalty, pad_token_id, streamer, constrained_processor=None):
        self.host_loops += 1
        return torch.cat([input_ids, torch.full_like(input_ids[:, :1], R.EOS)], dim=1)

    def _run_pt_single(self, formatted_prompt, temperature, cfg_scale, negative_prompt, top_k, top_p, repetition_penalty,
                       use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata, stop_at_reasoning,
                       skip_genres, skip_caption, skip_language, generation_phase, caption, lyrics, cot_text):
        assert not cfg_scale > 1.0 and use_constrained_decoding
        self.calls += 1
        proc = self._setup_constrained_processor(use_constrained_decoding, constrained_decoding_debug, target_duration, user_metadata,
                                                 stop_at_reasoning, skip_genres, skip_caption, skip_language, generation_phase, is_batch=False)
        tok = self.llm_tokenizer
        with self._load_model_context():
            inputs = tok(formatted_prompt, return_tensors="pt", padding=False, truncation=True)
            inputs = {k: v.to(self.device) for k, v in inputs.items()}
            max_new_tokens = self._compute_max_new_tokens(target_duration, generation_phase,
                                                          fallback_max=getattr(getattr(self.llm, "config", None), "max_new_tokens", 4096))
            out = self._generate_with_constrained_decoding(inputs["input_ids"], inputs.get("attention_mask"), max_new_tokens, temperature,
                                                           top_k, top_p, repetition_penalty, tok.pad_token_id or tok.eos_token_id, None, proc)
        return tok.decode(out[0][inputs["input_ids"].shape[1]:].cpu(), skip_special_tokens=False)


def _host(lm, device, nocfg=True):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, NoCfgHost):
        pass

    h = Handler(lm, device)
    h.use_native_lm_nocfg = nocfg
    return h


ARGS = dict(temperature=TEMP, cfg_scale=1.0, negative_prompt="NO USER INPUT", top_k=None, top_p=TOP_P, repetition_penalty=2.0,
            use_constrained_decoding=True, target_duration=1.2, generation_phase="codes", caption="c", lyrics="l", cot_text="t")


class _SequentialOnly:
    """The sequential path of a flag-on handler: ``nocfg_batch_request`` is told no for the length of the block."""

    def __enter__(self):
        from ace355 import lmlogits
        self.mod, self.old = lmlogits, lmlogits.nocfg_batch_request
        lmlogits.nocfg_batch_request = lambda *a, **k: (False, "the test asks for the sequential path")
        return self

    def __exit__(self, *exc):
        self.mod.nocfg_batch_request = self.old


def test_run_pt_batched_returns_the_sequential_strings(lms, gpu_device, caplog):
    lm = lms["bf16"]
    seeds = SEEDS[:5]
    h = _host(lm, gpu_device)
    with _SequentialOnly():                                      # item by item, each item the native loop seeded by _run_pt
        want = h._run_pt([S.COND_PROMPT] * 5, seeds=list(seeds), **ARGS)
    assert h.calls == 5 and h.host_loops == 0 and h._lm_loop_stats["steps"] == 7 and "batch" not in h._lm_loop_stats
    h = _host(lm, gpu_device)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="ace355"):
        got = h._run_pt([S.COND_PROMPT] * 5, seeds=list(seeds), **ARGS)
    assert got == want and len(set(got)) > 1 and all(t.endswith(str(R.EOS)) and len(t.split()) == 7 for t in got)
    assert h.calls == 0 and h.host_loops == 0 and h._lm_loop_stats["batch"] == 5 and h._lm_loop_stats["prefill_rows"] == 1
    assert not [r for r in caplog.records if "native-lm-nocfg" in r.getMessage() or "native-lm-batch" in r.getMessage()]
    assert h.setups == [(None, False, True, True, True, False)] and h.contexts == 1 and h.llm_tokenizer.sides == []
    assert h.constrained_processor.codes_count == 7
    off = _host(lm, gpu_device, nocfg=False)                     # the flag off: the host's own path, nothing said
    assert off._run_pt([S.COND_PROMPT] * 2, seeds=list(seeds[:2]), **ARGS) == [str(R.EOS)] * 2 and off.calls == 2 and off.host_loops == 2


def test_run_pt_goes_item_by_item_with_one_log_line_when_the_handle_does_not_fit(gpu_device, caplog):
    """A handle too small for the request (6 + 16 positions) and an fp16 ``out_dtype``: the batch is not tried, every item goes to
    the host's own loop, and the reason is said once."""
    from ace355.lm import NativeCausalLM
    caplog.set_level(logging.INFO, logger="ace355")
    for kw, word in ((dict(max_positions=16), "exceed the native handle"), (dict(max_positions=72, out_dtype=torch.float16), "out_dtype")):
        small = NativeCausalLM(L.TINY, gpu_device, max_seqs=4, **kw)
        try:
            small.load_state_dict(dict(L.weights("tiny")))
            caplog.clear()
            h = _host(small, gpu_device)
            assert h._run_pt([S.COND_PROMPT] * 3, seeds=SEEDS[:3], **ARGS) == [str(R.EOS)] * 3
            assert h.calls == 3 and h.host_loops == 3 and h._lm_loop_stats is None
            said = [r.getMessage() for r in caplog.records if "native-lm-nocfg" in r.getMessage()]
            assert len(said) == 1 and word in said[0] and "item by item" in said[0], said
        finally:
            small.close()


def test_run_pt_batched_runs_more_items_than_the_handle_holds_as_groups(gpu_device):
    from ace355.lm import NativeCausalLM
    small = NativeCausalLM(L.TINY, gpu_device, max_positions=32, max_seqs=2, out_dtype=torch.bfloat16)
    try:
        small.load_state_dict(dict(L.weights("tiny")))
        seeds = SEEDS[:5]
        h = _host(small, gpu_device)
        with _SequentialOnly():
            want = h._run_pt([S.COND_PROMPT] * 5, seeds=list(seeds), **ARGS)
        h = _host(small, gpu_device)
        assert h._run_pt([S.COND_PROMPT] * 5, seeds=list(seeds), **ARGS) == want
        assert h.calls == 0 and len(h.setups) == 3 and h._lm_loop_stats["batch"] == 1      # groups of 2, 2 and 1
        from ace355.lmlogits import generate_codes_batch_nocfg
        ids, am = NR.loop_prompt(1)
        with pytest.raises(ValueError, match="3 songs need 3 sequences, the native LM holds 2"):
            generate_codes_batch_nocfg(h, small, ids.to(gpu_device), am.to(gpu_device), [1, 2, 3], 16, TEMP, None, TOP_P, 1.0, R.PAD,
                                       R.make_processor(6, None))
    finally:
        small.close()
