"""GPU: the native logits stage (``ace355_lm_shape``) bit for bit against its numpy restatement (tests/_lm_logits_oracle.py, itself held
to the reference's output by G23), the seen-id bitmap, the decode step that takes device tokens, and the device-resident CFG loop
against the restated reference loop (tests/_lm_loop_ref.py) driven with the host-id decode, torch operations and ``select_tokens``."""
import ctypes as C

import numpy as np
import pytest
import torch

import _lm_logits_oracle as O
import _lm_loop_ref as R
import _lm_oracle as L

pytestmark = pytest.mark.gpu

REAL_V = 217205
NEG = float("-inf")


def _inputs(B, V, seed):
    """cond, uncond [B, V] (randn * 3 with -inf, signed zeros and a -inf pair planted), codes mask, "understand" mask, eos, history."""
    g = torch.Generator().manual_seed(seed)
    cond, uncond = (torch.randn(B, V, generator=g) * 3).numpy(), (torch.randn(B, V, generator=g) * 3).numpy()
    rng = np.random.default_rng(seed)
    for a in (cond, uncond):
        a[rng.random((B, V)) < 0.02] = -np.inf
        a[rng.random((B, V)) < 0.02] = -0.0
        a[rng.random((B, V)) < 0.01] = 0.0
    cond[:, V // 2] = uncond[:, V // 2] = -np.inf
    eos = V - 1 if V < 3 else V - 3
    mask = np.where(rng.random(V) < 0.5, 0.0, -np.inf).astype(np.float32)
    mask[eos] = 0.0
    amask = np.where(mask == 0, -np.inf, 0.0).astype(np.float32)
    hist = rng.integers(-2, V + 2, size=(B, 40))
    hist[:, 1] = hist[:, 0]
    return cond, uncond, mask, amask, eos, hist


def _settings():
    """Every processor branch of G23 (a) with the three temperatures and penalties cycling through them; cfg_scale 1.7 throughout."""
    temps, pens = (None, 0.7, 0.0), (1.0, 1.1, 1.3)
    return [(m, temps[(i + j) % 3], pens[(2 * i + j) % 3]) for i, m in enumerate(O.MODE_NAMES) for j in range(2)]


def _bits_equal(got: torch.Tensor, want: np.ndarray, what):
    got = got.detach().cpu().numpy()
    if not O.same_bits(got, want):
        bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        r, v = bad[0]
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at row {r} id {v}: {got[r, v]!r} vs {want[r, v]!r}")


def _native(dev, cond, uncond, mask, amask, eos, hist, mode, T, pen, layout="dense"):
    from ace355.lmlogits import SeenTokens, shape_logits
    B, V = cond.shape
    which, eos_mode = O.MODES[mode]
    m = {"codes": mask, "audio": amask, None: None}[which]

    def put(a):
        if layout != "strided":
            return torch.from_numpy(a).to(dev)
        wide = torch.full((B, V + 13), float("nan"), device=dev)   # rows strided out of a wider NaN-filled tensor, base off 16 bytes
        wide[:, 5:5 + V] = torch.from_numpy(a).to(dev)
        return wide[:, 5:5 + V]
    c, u = put(cond), put(uncond) if uncond is not None else None
    seen = SeenTokens(B, V, dev).mark(torch.from_numpy(hist).to(dev)) if pen != 1.0 else None
    out = c if layout == "alias" else (put(np.zeros_like(cond)) if layout == "strided" else None)
    got = shape_logits(c, u, O.CFG_SCALE, torch.from_numpy(m).to(dev) if m is not None else None, eos if eos_mode else None, eos_mode, T, pen,
                       seen, out=out)
    if layout == "alias":
        assert got.data_ptr() == c.data_ptr()
    return got


def _want(cond, uncond, mask, amask, eos, hist, mode, T, pen):
    which, eos_mode = O.MODES[mode]
    m = {"codes": mask, "audio": amask, None: None}[which]
    return O.shape(cond, uncond, O.CFG_SCALE, m, eos, eos_mode, T, pen, O.seen_bitmap(hist, cond.shape[1]))


# ------------------------------------------------------------------ the stage
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 8191, 8192, 8193, 2 * 8192 + 1])
def test_shape_equals_the_oracle_bit_for_bit(gpu_device, V, B):
    """Chunk edges of plan_lm_pick (8192), head / tail of the 16-byte groups (odd V: every row has another alignment), every branch."""
    a = _inputs(B, V, 100 * V + B)
    for i, (mode, T, pen) in enumerate(_settings()):
        layout = ("dense", "strided", "alias")[i % 3]
        _bits_equal(_native(gpu_device, *a, mode, T, pen, layout), _want(*a, mode, T, pen), (V, B, mode, T, pen, layout))
    cond, _u, *rest = a                                           # uncond NULL: no CFG
    for layout in ("dense", "strided", "alias"):
        _bits_equal(_native(gpu_device, cond, None, *rest, "block", 0.7, 1.3, layout), _want(cond, None, *rest, "block", 0.7, 1.3),
                    (V, B, "no uncond", layout))


def test_shape_strided_rows_leave_the_gaps_alone(gpu_device):
    from ace355.lmlogits import shape_logits
    B, V = 3, 8193
    cond, uncond, mask, _am, eos, _h = _inputs(B, V, 7)
    wide = torch.full((B, V + 11), float("nan"), device=gpu_device)
    out = wide[:, 3:3 + V]
    shape_logits(torch.from_numpy(cond).to(gpu_device), torch.from_numpy(uncond).to(gpu_device), O.CFG_SCALE,
                 torch.from_numpy(mask).to(gpu_device), eos, O.EOS_BLOCK, 0.7, out=out)
    _bits_equal(out, O.shape(cond, uncond, O.CFG_SCALE, mask, eos, O.EOS_BLOCK, 0.7), "strided out")
    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + V:]).all()


def test_shape_row_does_not_depend_on_batch_or_neighbours(gpu_device):
    B, V = 16, 8193
    a = _inputs(B, V, 11)
    cond, uncond, mask, amask, eos, hist = a
    full = _native(gpu_device, *a, "block", 0.7, 1.3).cpu().numpy()
    for r in (0, 5, 15):
        alone = _native(gpu_device, cond[r:r + 1], uncond[r:r + 1], mask, amask, eos, hist[r:r + 1], "block", 0.7, 1.3)
        _bits_equal(alone, full[r:r + 1], f"row {r} alone")
    c2, u2, h2 = np.full_like(cond, np.nan), np.full_like(uncond, np.nan), np.zeros_like(hist)
    c2[5], u2[5], h2[5] = cond[5], uncond[5], hist[5]
    _bits_equal(_native(gpu_device, c2, u2, mask, amask, eos, h2, "block", 0.7, 1.3)[5:6], full[5:6], "row 5 among NaN rows")


def test_shape_at_the_real_vocabulary(gpu_device):
    a = _inputs(2, REAL_V, 2051)
    for mode, T, pen, layout in (("block", 0.7, 1.3, "dense"), ("force", None, 1.1, "alias"), ("understand", 0.0, 1.0, "strided")):
        _bits_equal(_native(gpu_device, *a, mode, T, pen, layout), _want(*a, mode, T, pen), (mode, T, pen, layout))


def test_shape_python_checks(gpu_device):
    from ace355.lmlogits import shape_logits
    x = torch.zeros(2, 10, device=gpu_device)
    for bad in (x.double(), x.cpu(), x[:, ::2], x[0]):
        with pytest.raises(ValueError):
            shape_logits(bad)
    with pytest.raises(ValueError):
        shape_logits(x, x[:1])
    with pytest.raises(ValueError):
        shape_logits(x, penalty=1.2)                             # no SeenTokens
    with pytest.raises(ValueError):
        shape_logits(x, mask=torch.zeros(11, device=gpu_device))
    with pytest.raises(RuntimeError, match="eos_id"):
        shape_logits(x, eos_id=10, eos_mode=O.EOS_BLOCK)


# ------------------------------------------------------------------ the bitmap
def test_seen_mark_equals_a_numpy_bitmap(gpu_device):
    from ace355.lmlogits import SeenTokens
    B, V = 3, 1003
    rng = np.random.default_rng(3)
    a, b = rng.integers(-5, V + 5, size=(B, 300)), rng.integers(0, V, size=(B, 1))
    a[:, 10:20] = a[:, :10]                                      # duplicates
    a[0, 0], a[0, 1], a[1, 0] = V, -1, 2 ** 40                   # out of range: ignored
    a[2, :] = 64                                                 # one row marks a single id
    seen = SeenTokens(B, V, gpu_device)
    assert seen.words.shape == (B, 32) and not seen.words.any()
    wide = torch.from_numpy(np.concatenate([a, a], 1)).to(gpu_device)
    seen.mark(wide[:, :300])                                     # strided rows
    got = seen.words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, O.seen_bitmap(a, V)) and got[2].tolist() == [0, 0, 1] + [0] * 29
    seen.mark(torch.from_numpy(b[:, 0]).to(gpu_device))          # a second call accumulates; [B] is [B, 1]
    assert np.array_equal(seen.words.cpu().numpy().view(np.uint32), O.seen_bitmap(np.concatenate([a, b], 1), V))
    with pytest.raises(ValueError):
        seen.mark(wide[:2])
    with pytest.raises(ValueError):
        seen.mark(wide.int())


# ------------------------------------------------------------------ decode_tokens
@pytest.fixture(scope="module")
def lm(gpu_device):
    from ace355.lm import NativeCausalLM
    w = L.weights("tiny")
    lm = NativeCausalLM(L.TINY, gpu_device, max_positions=64, max_seqs=4)
    lm.load_state_dict(dict(w))
    yield lm
    lm.close()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_decode_tokens_equals_decode(lm, gpu_device):
    V = L.TINY.vocab_size
    ids, first = L.left_padded([6, 3, 5, 2], 6, V, 31)
    am = L.mask_of(first, 6)
    nxt = torch.tensor([5, 900, 17, 1002])
    lm.prefill(ids, am)
    want = [lm.decode(nxt), lm.decode(nxt.flip(0))]
    lm.prefill(ids, am)
    got = [lm.decode_tokens(nxt.to(gpu_device)), lm.decode_tokens(nxt.flip(0).to(gpu_device))]
    assert lm.length == 8 and lm.bad_tokens() == 0
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w))
    lm.prefill(ids, am)                                          # B = N / 2: sequence n takes tokens[n % B]
    want = lm.decode(torch.tensor([5, 900, 5, 900]))
    lm.prefill(ids, am)
    assert torch.equal(_bits(lm.decode_tokens(torch.tensor([5, 900], device=gpu_device))), _bits(want))
    assert lm.bad_tokens() == 0


def test_decode_tokens_counts_a_bad_token_and_goes_on(lm, gpu_device):
    V = L.TINY.vocab_size
    ids, first = L.left_padded([6, 3, 5, 2], 6, V, 32)
    am = L.mask_of(first, 6)
    lm.prefill(ids, am)
    clean = lm.decode(torch.tensor([5, 9, 5, 9]))
    lm.prefill(ids, am)
    zero = lm.decode(torch.tensor([5, 0, 5, 0]))
    lm.prefill(ids, am)
    got = lm.decode_tokens(torch.tensor([5, V + 3], device=gpu_device))       # sequences 1 and 3 get id 0 in its place
    nxt = lm.decode_tokens(torch.tensor([-1, 7], device=gpu_device))
    assert torch.isfinite(nxt).all()
    assert lm.bad_tokens() == 4 and lm.bad_tokens() == 0
    assert torch.equal(_bits(got[0::2]), _bits(clean[0::2])) and torch.equal(_bits(got), _bits(zero))
    lm.prefill(ids, am)                                          # the next good call is clean
    assert torch.equal(_bits(lm.decode_tokens(torch.tensor([5, 9], device=gpu_device))), _bits(clean)) and lm.bad_tokens() == 0


def test_decode_tokens_refusals(lm, gpu_device):
    from ace355 import native
    from ace355.lm import NativeCausalLM
    V = L.TINY.vocab_size
    ids, first = L.left_padded([6, 3, 5, 2], 6, V, 33)
    lm.prefill(ids, L.mask_of(first, 6))
    tok = torch.tensor([1, 2, 3], device=gpu_device)
    out = torch.empty(4, V, device=gpu_device)
    lib = native.lib()
    for B in (3, 0, -1, 8):
        assert lib.ace355_lm_decode_tokens(lm._h, tok.data_ptr(), B, out.data_ptr(), None) == 1 and "lm_decode_tokens" in native.last_error()
    assert lm.length == 6                                        # refused with the handle unchanged
    for bad in (tok, tok[:2].int(), tok[:2].cpu(), tok[:2, None]):
        with pytest.raises(ValueError):
            lm.decode_tokens(bad)
    small = NativeCausalLM(L.TINY, gpu_device, max_positions=7, max_seqs=2)
    try:
        small.load_state_dict(dict(L.weights("tiny")))
        assert lib.ace355_lm_decode_tokens(small._h, tok.data_ptr(), 1, out.data_ptr(), None) == 1 and "no prefill" in native.last_error()
        assert small.bad_tokens() == 0
        small.prefill(ids[:2], L.mask_of(first[:2], 6))
        small.decode_tokens(tok[:1])
        assert lib.ace355_lm_decode_tokens(small._h, tok.data_ptr(), 1, out.data_ptr(), None) == 1 and "full" in native.last_error()
        with pytest.raises(ValueError):
            small.decode_tokens(tok[:1])
    finally:
        small.close()


# ------------------------------------------------------------------ the loop
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

    def _generate_with_cfg_custom(self, *a, **k):
        raise AssertionError("the reference's loop must not be asked")


def _handler(lm, gpu_device):
    from ace355.backend import NativeLmMixin

    class Handler(NativeLmMixin, _RefBase):
        pass

    h = Handler()
    h.llm, h.device, h.use_native_lm_loop = lm, gpu_device, True
    h.llm_tokenizer = R.FakeTokenizer(R.EOS)
    return h


TOP_P, TEMP, CFG = 0.9, 0.85, 2.0


def _both(lm, gpu_device, B, target, pair, max_new, streamer=False, seed=5):
    """(native ids, stats, processor, streamer), (reference ids, processor, streamer) for the same prompt, settings and torch seed."""
    from ace355 import lmsample
    pen, T = (2.0, 0.5) if pair else (1.0, None)
    ids, am = R.loop_prompt(B)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    h = _handler(lm, gpu_device)
    p1, s1 = R.make_processor(target, T), _Streamer() if streamer else None
    torch.manual_seed(seed)
    got = h._generate_with_cfg_custom(ids, am, max_new, TEMP, CFG, None, TOP_P, pen, R.PAD, s1, p1)
    p2, s2 = R.make_processor(target, T), _Streamer() if streamer else None
    torch.manual_seed(seed)
    with torch.inference_mode():
        want = R.run_loop(lambda g, step: lm.prefill(g, am) if step == 0 else lm.decode(g[:, -1]), R.torch_stage(CFG, pen),
                          lambda x: lmsample.select_tokens(x, None, TOP_P, TEMP), ids, max_new, R.EOS, R.PAD, p2, s2)
    return (got, h._lm_loop_stats, p1, s1), (want, p2, s2)


@pytest.mark.parametrize("pair", [False, True], ids=["plain", "penalty2_T0.5"])
@pytest.mark.parametrize("target", [6, 10])
@pytest.mark.parametrize("B", [1, 2])
def test_loop_with_a_target_matches_and_reads_two_tokens(lm, gpu_device, B, target, pair):
    (got, stats, p1, _s), (want, p2, _s2) = _both(lm, gpu_device, B, target, pair, 14)
    assert got.dtype == want.dtype and got.device == want.device and torch.equal(got, want)
    steps = -(-target // B) + 1
    assert got.shape == (2 * B, 6 + steps) and (got[:, -1] == R.EOS).all() and torch.equal(got[:B, 6:], got[B:, 6:])
    assert ((got[:B, 6:-1] >= 300) & (got[:B, 6:-1] < 900)).all()
    assert p1.state == p2.state == R.FSMState.CODES_GENERATION and p1.codes_count == p2.codes_count == B * steps
    assert stats["steps"] == steps and stats["native_steps"] == steps - 1
    assert stats["token_reads"] <= 2 and stats["sync_free_steps"] == stats["native_steps"] - 1


@pytest.mark.parametrize("B", [1, 2])
def test_loop_with_a_streamer_or_without_a_target_reads_every_step(lm, gpu_device, B):
    (got, stats, p1, s1), (want, p2, s2) = _both(lm, gpu_device, B, 6, True, 14, streamer=True)
    assert torch.equal(got, want) and p1.codes_count == p2.codes_count
    assert stats["sync_free_steps"] == 0 and stats["token_reads"] == stats["steps"] == got.shape[1] - 6
    assert s1.ended == s2.ended == 1 and len(s1.put_calls) == len(s2.put_calls) == stats["steps"]
    assert all(torch.equal(a, b) and a.shape == (B, 1) for a, b in zip(s1.put_calls, s2.put_calls))
    (got, stats, p1, _s), (want, p2, _s2) = _both(lm, gpu_device, B, None, False, 8)
    assert torch.equal(got, want) and p1.codes_count == p2.codes_count and p1.state == p2.state
    assert stats["sync_free_steps"] == 0 and stats["token_reads"] == stats["steps"] == got.shape[1] - 6


def test_loop_without_a_processor(lm, gpu_device):
    """No constrained processor: every step is native, reads its tokens, and the ids are the restated loop's."""
    from ace355 import lmsample
    ids, am = R.loop_prompt(2)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    h = _handler(lm, gpu_device)
    torch.manual_seed(9)
    got = h._generate_with_cfg_custom(ids, am, 5, TEMP, CFG, None, TOP_P, 2.0, R.PAD, None, None)
    torch.manual_seed(9)
    with torch.inference_mode():
        want = R.run_loop(lambda g, step: lm.prefill(g, am) if step == 0 else lm.decode(g[:, -1]), R.torch_stage(CFG, 2.0),
                          lambda x: lmsample.select_tokens(x, None, TOP_P, TEMP), ids, 5, R.EOS, R.PAD, None)
    assert torch.equal(got, want)
    assert h._lm_loop_stats["native_steps"] == h._lm_loop_stats["token_reads"] == h._lm_loop_stats["steps"] == got.shape[1] - 6


def test_loop_runs_on_a_handle_made_for_plain_cuda(gpu_device, caplog):
    """``LLMHandler.initialize`` stores the device as "cuda", without an index, and that string is what the native LM is built with;
    tensors report "cuda:0".  The handle must name the device it is on, or the override would hand every request to the reference's
    loop and ``decode_tokens`` would refuse its tokens."""
    import logging
    from ace355.lm import NativeCausalLM
    plain = NativeCausalLM(L.TINY, "cuda", max_positions=64, max_seqs=4)
    try:
        assert plain.device.index is not None and plain.device == torch.device("cuda", torch.cuda.current_device())
        plain.load_state_dict(dict(L.weights("tiny")))
        h = _handler(plain, "cuda")
        ids, am = R.loop_prompt(2)
        ids, am = ids.to("cuda"), am.to("cuda")
        proc = R.make_processor(6, None)
        torch.manual_seed(5)
        with caplog.at_level(logging.INFO, logger="ace355"):
            got = h._generate_with_cfg_custom(ids, am, 14, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, proc)
        assert not [r for r in caplog.records if "native-lm-loop" in r.getMessage()]
        stats = h._lm_loop_stats
        assert stats["steps"] == 4 and stats["native_steps"] == 3 and stats["sync_free_steps"] == 2 and stats["token_reads"] == 2
        assert got.shape == (4, 10) and (got[:, -1] == R.EOS).all() and proc.codes_count == 8
        assert plain.decode_tokens(torch.tensor([5, 9], device="cuda")).shape == (4, L.TINY.vocab_size) and plain.bad_tokens() == 0
    finally:
        plain.close()


class _StubLm:
    """What generate_with_cfg asks of a NativeCausalLM, with logits that turn NaN at one step."""
    out_dtype = torch.float32
    cfg = L.TINY

    def __init__(self, dev, nan_step):
        self.dev, self.nan_step, self.step, self.fed = dev, nan_step, 0, []

    def _logits(self, N):
        x = torch.randn(N, L.TINY.vocab_size, device=self.dev)
        if self.step == self.nan_step:
            x[0, 400] = float("nan")
        self.step += 1
        return x

    def prefill(self, ids, mask):
        return self._logits(ids.shape[0])

    def decode_tokens(self, tokens):
        self.fed.append(tokens.clone())
        return self._logits(2 * tokens.shape[0])

    def bad_tokens(self):
        return 0


@pytest.mark.parametrize("sync_free", [False, True])
def test_loop_raises_when_a_step_could_draw_no_token(gpu_device, sync_free):
    """A NaN row gives token -1 (as data).  On a step that reads its tokens the loop stops there; on a sync-free step nothing is read,
    the loop runs on and the check after it raises.  Either way it raises instead of returning ids: the processor has moved."""
    from ace355.lmlogits import generate_with_cfg
    ids, am = R.loop_prompt(2)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    h = _RefBase()
    h.llm_tokenizer = R.FakeTokenizer(R.EOS)
    stub = _StubLm(gpu_device, nan_step=2)
    proc = R.make_processor(40, None) if sync_free else None
    torch.manual_seed(1)
    with pytest.raises(RuntimeError, match="no valid token"):
        generate_with_cfg(h, stub, ids, am, 6, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, proc)
    if sync_free:
        assert h._lm_loop_stats["steps"] == 6 and h._lm_loop_stats["token_reads"] == 1 and proc.codes_count == 12
        assert stub.fed[2][0].item() == -1 and (stub.fed[2][1] >= 300).item()
    else:
        assert h._lm_loop_stats["steps"] == 3 and len(stub.fed) == 2


def test_loop_goes_to_the_reference_when_the_handle_is_too_small(lm, gpu_device, caplog):
    """Each precondition sends the whole call to the reference's loop, and says why, once per reason."""
    import logging
    from ace355.backend import NativeLmMixin
    caplog.set_level(logging.INFO, logger="ace355")

    class Base:
        def _generate_with_cfg_custom(self, *a):
            return "reference"

    class Handler(NativeLmMixin, Base):
        pass

    h = Handler()
    h.llm, h.device, h.use_native_lm_loop = lm, gpu_device, True
    ids, am = R.loop_prompt(2)
    ids, am = ids.to(gpu_device), am.to(gpu_device)
    assert h._generate_with_cfg_custom(ids, am, 64, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, None) == "reference"      # P + new > max_positions
    big = torch.cat([ids, ids, ids], 0)
    assert h._generate_with_cfg_custom(big, None, 4, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, None) == "reference"     # 2B > max_seqs
    holes = am.clone()
    holes[0, 2] = 0
    assert h._generate_with_cfg_custom(ids, holes, 4, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, None) == "reference"    # not left-padded
    assert h._generate_with_cfg_custom(ids, holes, 4, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, None) == "reference"    # (logged once)
    h.llm = object()
    assert h._generate_with_cfg_custom(ids, am, 4, TEMP, CFG, None, TOP_P, 1.0, R.PAD, None, None) == "reference"       # not the native LM
    said = [r.getMessage() for r in caplog.records if "native-lm-loop" in r.getMessage()]
    assert len(said) == 4 and "exceed the native handle" in said[0] and "exceed the native handle" in said[1] and said[0] != said[1]
    assert "left-padded" in said[2] and "not the native LM" in said[3]
