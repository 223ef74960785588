"""CPU: the lyric alignment stage after the maps - the CPU restatement (tests/_lyric_post_ref.py) against the reference's recorded
results (tests/golden/g20_lyric_post.npz), the host-side text pieces of ace355.align_post, the ABI, and the mixin's opt-in on stub hosts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ace355
from ace355 import align_post
from ace355.backend import NativeDitMixin, NativeHandler

import _lyric_post_ref as ref

TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)
TAGS = (("f32", torch.float32), ("bf16", torch.bfloat16))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_lyric_post.npz"))


def case_maps(G, c):
    """The fp32 ridge maps [H, R, S] of fixture case c, checked against the recorded checksums (case 0: against the stored maps)."""
    H, R, S = (int(v) for v in G["cases"][c])
    m = ref.ridge_maps(H, R, S, int(G["seed0"]) + c)
    if c == 0:
        assert np.array_equal(m.numpy(), G["c0_maps"])
    assert float(m.double().sum()) == pytest.approx(float(G[f"c{c}_maps_sum"]), rel=1e-12)
    weights = torch.arange(1, m.numel() + 1).reshape(m.shape).double()
    assert float((m.double() * weights).sum()) == pytest.approx(float(G[f"c{c}_maps_abs_sum"]), rel=1e-12)
    return m


def close(a, b, tol=1e-6):
    """max |a - b| within tol of the fixture's own maximum (another CPU's libm may differ in the last bit)."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) <= tol * float(np.abs(b).max())


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("tag,dt", TAGS)
def test_ref32_reproduces_the_timestamp_fixture(G, c, tag, dt):
    k = f"c{c}_{tag}_"
    maps = case_maps(G, c).to(dt).float()
    calc, energy = ref.timestamp_matrix(maps, 2.0, 1)
    assert close(calc, G[k + "ts_calc"]) and close(energy, G[k + "ts_energy"])
    rows, cols = ref.dtw(-calc.astype(np.float64))
    assert np.array_equal(np.stack([rows, cols]), G[k + "ts_path"])
    # the host-side pieces, from the path: token and sentence timestamps, LRC text
    tok = ref.ToyTokenizer()
    ids = ref.ToyTokenizer.ids(maps.shape[1])
    frames = ref.token_frames(rows, cols, maps.shape[1])
    toks = align_post.token_timestamps(tok, ids, frames.tolist(), maps.shape[2], float(G["duration"]))
    assert [t.start for t in toks] == G[k + "tok_start"].tolist() and [t.end for t in toks] == G[k + "tok_end"].tolist()
    assert [t.text for t in toks] == G[k + "tok_text"].tolist() and [t.token_id for t in toks] == ids
    sents = align_post.sentence_timestamps(tok, toks)
    assert [s.text for s in sents] == G[k + "sent_text"].tolist()
    assert [s.start for s in sents] == G[k + "sent_start"].tolist() and [s.end for s in sents] == G[k + "sent_end"].tolist()
    assert [s.confidence for s in sents] == G[k + "sent_conf"].tolist()
    assert align_post.format_lrc(sents) == str(G[k + "lrc"])


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("tag,dt", TAGS)
def test_ref32_reproduces_the_score_fixture(G, c, tag, dt):
    k = f"c{c}_{tag}_"
    maps = case_maps(G, c).to(dt).float()
    calc, energy = ref.score_matrix(maps, 1)
    if c < 2:
        assert close(energy, G[k + "sc_energy"])
    else:
        assert close(energy[::3, ::3], G[k + "sc_energy_sub3"])
    rows, cols = ref.dtw(-calc.astype(np.float32))
    path = np.stack([rows, cols], 1)
    assert np.array_equal(path, G[k + "sc_path"])
    ids = ref.ToyTokenizer.ids(maps.shape[1])
    mask = ref.type_mask(ref.ToyTokenizer(), ids)
    assert np.array_equal(mask, G[k + "sc_mask"]) and align_post.token_type_mask(ref.ToyTokenizer(), ids) == mask.tolist()
    met = ref.score_metrics(energy, path, mask)
    assert np.allclose(met, G[k + "sc_metrics"], rtol=1e-6, atol=0)
    assert ref.final_score(*met) == float(G[k + "sc_score"]) == align_post.final_score(*met)


def test_ref32_reproduces_the_tie_path(G):
    rows, cols = ref.dtw(G["ties_x"].astype(np.float64))
    assert np.array_equal(np.stack([rows, cols]), G["ties_path"])
    # the anti-diagonal order against the plain column-by-column loop, ties and all
    x = G["ties_x"]
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.zeros((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            c, t = (c0, 0) if c0 < c1 and c0 < c2 else (c1, 1) if c1 < c0 and c1 < c2 else (c2, 2)
            cost[i, j], trace[i, j] = np.float32(x[i - 1, j - 1]) + c, t
    i, j, path = N, M, []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = 2 if i == 0 else 1 if j == 0 else trace[i, j]
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    assert path[::-1] == list(zip(rows.tolist(), cols.tolist()))


def test_median_filter_and_ref64():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 5, 9, generator=g)
    assert torch.equal(ref.median_filter(x, 1), x) and ref.median_filter(x[..., :3], 7) is not None
    assert torch.equal(ref.median_filter(x[..., :3], 7), x[..., :3])        # S <= w // 2: the identity
    y = ref.median_filter(x, 3)
    assert y.shape == x.shape and float(y[0, 0, 0]) == float(torch.stack([x[0, 0, 1], x[0, 0, 0], x[0, 0, 1]]).median())
    m = ref.ridge_maps(3, 20, 33, 5)
    c32, e32 = ref.timestamp_matrix(m, 2.0, 3)
    c64, e64 = ref.timestamp_matrix(m, 2.0, 3, dtype=torch.float64)
    assert c64.dtype == np.float64 and np.abs(c32 - c64).max() < 1e-4 * np.abs(c64).max()
    assert np.abs(e32 - e64).max() < 1e-5 * np.abs(e64).max()


def test_host_pieces_edge_cases():
    tok = ref.ToyTokenizer()
    # a token split over two byte-level tokens lands whole on the one that completes it
    assert align_post.decode_tokens_incrementally(tok, [0, 6, 7, 2]) == ["la", "\ufffd", "", "\n"]
    # tokens off the path start and end where the previous one ended
    toks = align_post.token_timestamps(tok, [0, 1, 2], [(-1, -1), (2, 4), (-1, -1)], 10, 5.0)
    assert [(t.start, t.end) for t in toks] == [(0.0, 0.0), (1.0, 2.0), (2.0, 2.0)]
    assert align_post.token_type_mask(tok, [0, 3, 4, 5, 0, 5, 3]) == [1, 0, 0, 0, 1, 0, 0]
    T, S = align_post.payload_types()
    assert T is align_post.TokenTimestamp and S is align_post.SentenceTimestamp     # no acestep here
    s = [S(text="x", start=61.239, end=70.0, tokens=[], confidence=0.0)]
    assert align_post.format_lrc(s) == "[01:01.24]x"


def test_abi_symbols_and_signatures():
    from ace355 import native
    lib = native.lib()
    want = {"ace355_align_workspace_bytes": 4, "ace355_align_timestamp_matrix": 16, "ace355_align_score_matrix": 15,
            "ace355_align_dtw": 11, "ace355_align_score_metrics": 14, "ace355_align_median": 6}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ace355.h")).read()
    for name, nargs in want.items():
        res, args = native.SIGNATURES[name]
        assert hasattr(lib, name) and len(args) == nargs
        decl = header[header.index(name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs, name
    assert native.SIGNATURES["ace355_align_workspace_bytes"][0] is ctypes.c_size_t
    # sizes and argument checks run on the host: no GPU needed
    assert lib.ace355_align_workspace_bytes(7, 769 - 12, 750, 2) >= 7 * 757 * 750 * 4
    assert lib.ace355_align_workspace_bytes(0, 5, 5, 1) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    ts = lib.ace355_align_timestamp_matrix
    good = dict(maps=p, P=2, N=2, L=8, S=4, n=1, row0=2, rows=3, v=2.0, w=1, rb=0, calc=p, energy=p, ws=p, nbytes=big, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return ts(a["maps"], a["P"], a["N"], a["L"], a["S"], a["n"], a["row0"], a["rows"], a["v"], a["w"], a["rb"], a["calc"], a["energy"],
                  a["ws"], a["nbytes"], a["stream"])
    for bad in (dict(maps=None), dict(ws=None), dict(rows=0), dict(S=0), dict(row0=6), dict(row0=-1), dict(n=2), dict(n=-1), dict(w=2),
                dict(w=33), dict(rows=8193, L=9000), dict(S=16385), dict(nbytes=16), dict(P=65)):
        assert call(**bad) == 1, bad
        assert "align_timestamp_matrix" in native.last_error()
    assert lib.ace355_align_dtw(p, 1, 8193, 4, -1.0, p, p, p, p, big, None) == 1
    assert lib.ace355_align_dtw(p, 1, 4, 4, -1.0, p, p, p, p, 8, None) == 1 and "workspace" in native.last_error()
    assert lib.ace355_align_score_metrics(p, p, p, None, 1, 4, 4, 0.01, 9.0, 1.0, p, p, big, None) == 1
    assert lib.ace355_align_score_matrix(p, 2, 2, 8, 4, 1, 2, 3, 4, 0, p, p, p, big, None) == 1
    assert lib.ace355_align_median(p, 1, 0, 1, p, None) == 1


# ------------------------------------------------------------------------------------------------ the mixin's opt-in on a stub host
def _maps(P, N, L, S):
    return torch.softmax(torch.randn(P, N, S, L, generator=torch.Generator().manual_seed(1)), -1).transpose(-1, -2).contiguous()


class _FakeDit:
    def __init__(self):
        self.cfg = ace355.DitConfig(**TINY)
        self.device = torch.device("cpu")
        self.calls = 0

    def set_condition(self, slot, enc, L=None):
        pass

    def cross_attention_maps(self, x, ctx, t, t_r, slots, prs):
        self.calls += 1
        return _maps(len(prs), x.shape[0], 12, (x.shape[1] + 1) // 2)


class _Host(NativeDitMixin):
    def __init__(self):
        self.native_dit, self.use_native_dit = _FakeDit(), True
        self.device, self.dtype = "cpu", torch.bfloat16
        self.text_tokenizer = ref.ToyTokenizer()


def _args():
    g = torch.Generator().manual_seed(7)
    return dict(pred_latent=torch.randn(1, 9, 64, generator=g), encoder_hidden_states=torch.randn(1, 12, 256, generator=g),
                encoder_attention_mask=torch.ones(1, 12), context_latents=torch.randn(1, 9, 128, generator=g),
                lyric_token_ids=torch.tensor([[0, 1, 2, 3, 4, 0, 1, 9, 2, 8, 151643, 0]]), custom_layers_config={0: [1], 1: [0, 1]})


@pytest.fixture
def host_scoring(monkeypatch):
    for k, v in ref.fake_scoring_modules().items():
        monkeypatch.setitem(sys.modules, k, v)


@pytest.fixture
def spy(monkeypatch):
    """Every device entry point of ace355.align_post raises and is counted."""
    hits = []

    def boom(name):
        def f(*a, **k):
            hits.append(name)
            raise RuntimeError("native stage failure")
        return f
    for name in ("timestamp_matrix", "score_matrix", "dtw_raw", "dtw", "score_metrics", "lyric_timestamps", "lyric_scores"):
        monkeypatch.setattr(align_post, name, boom(name))
    return hits


def test_opt_in_is_off_by_default_and_then_nothing_new_runs(host_scoring, spy):
    assert NativeDitMixin.native_lyric_post is False and NativeHandler().native_lyric_post is False
    host = _Host()
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0)
    assert r["success"] is True and r["lrc_text"] and not spy and host.native_dit.calls == 1
    r = host.get_lyric_score(**_args())
    assert r["success"] is True and not spy


def test_opt_in_with_a_failing_native_stage_runs_the_host_aligner(host_scoring, spy):
    off = _Host()
    want_ts = off.get_lyric_timestamp(**_args(), total_duration_seconds=30.0)
    want_sc = off.get_lyric_score(**_args())
    host = _Host()
    host.native_lyric_post = True
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0)
    assert spy == ["lyric_timestamps"] and r["success"] is True
    assert r["lrc_text"] == want_ts["lrc_text"] and r["token_timestamps"] == want_ts["token_timestamps"]
    r = host.get_lyric_score(**_args())
    assert spy == ["lyric_timestamps", "lyric_scores"] and r == want_sc and 0.0 <= r["lm_score"] <= 1.0


def test_opt_in_without_a_scoring_package_reports_the_host_error(monkeypatch, spy):
    monkeypatch.setitem(sys.modules, "acestep", None)
    host = _Host()
    host.native_lyric_post = True
    r = host.get_lyric_timestamp(**_args(), total_duration_seconds=30.0)
    assert r["success"] is False and r["error"].startswith("Error generating timestamps:") and spy == ["lyric_timestamps"]


def test_env_switch_is_read_once_at_import():
    import subprocess
    code = "import ace355.backend as b; print(b.NativeDitMixin.native_lyric_post, b.NativeHandler().native_lyric_post)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACE355_ALIGN_POST="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", "import ace355\n" + code], env=env, cwd=root, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["True", "True"]
