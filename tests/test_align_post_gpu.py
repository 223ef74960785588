"""GPU: the lyric alignment stage after the maps (ace355_align_*, csrc/align_post.hip) - exact medians, the timestamp / score matrices
under the 8(d) rule against fp64, the DTW bit for bit against the sequential fp32 code, the fp64 metrics, the whole stage on the
reference's recorded cases (tests/golden/g20_lyric_post.npz) and the handler opt-in on the tiny DiT."""
import os
import sys

import numpy as np
import pytest
import torch

import _lyric_post_ref as ref

pytestmark = pytest.mark.gpu

TAGS = (("f32", torch.float32), ("bf16", torch.bfloat16))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_lyric_post.npz"))


def rel(a, b):
    """max |a - b| / max |b| (0 when both vanish)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d, m = float(np.abs(a - b).max()), float(np.abs(b).max())
    return d / m if m > 0 else d


# ------------------------------------------------------------------------------------------------ 1. medians
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129, 750, 1025, 2049, 8194])
def test_median_is_torch_quantile_bit_for_bit(gpu_device, n):
    """8194 is past the line length staged in LDS: the selection then reads global memory."""
    from ace355 import align_post
    g = torch.Generator().manual_seed(n)
    lines = [torch.rand(n, generator=g), torch.randn(n, generator=g), torch.full((n,), 0.37), torch.zeros(n)]
    mostly_zero = torch.rand(n, generator=g) * (torch.rand(n, generator=g) > 0.9)
    dup = torch.rand(n, generator=g)
    srt = dup.sort().values
    dup = torch.where((dup >= srt[max(0, (n - 1) // 2 - 1)]) & (dup <= srt[min(n - 1, n // 2 + 1)]), srt[(n - 1) // 2], dup)   # duplicates straddling the middle
    few = torch.randint(0, 3, (n,), generator=g).float()
    x = torch.stack(lines + [mostly_zero, dup, few, dup[torch.randperm(n, generator=g)]])       # [8, n]
    for t, dim in ((x, 1), (x.t().contiguous(), 0), (x[:, :, None].expand(-1, -1, 3).contiguous(), 1)):
        got = align_post.median(t.to(gpu_device), dim).cpu()
        want = torch.quantile(t, 0.5, dim)
        assert got.shape == want.shape and torch.equal(got, want), (n, dim, float((got - want).abs().max()))


# ------------------------------------------------------------------------------------------------ 2. timestamp / score matrices
def embed(block, gpu_device, row0=3, tail=2):
    """[H, R, S] as item 1 of N = 2, rows [row0, row0 + R) of a longer L, everything else other positive values."""
    H, R, S = block.shape
    g = torch.Generator().manual_seed(R + S)
    maps = torch.rand(H, 2, row0 + R + tail, S, generator=g)
    maps[:, 1, row0:row0 + R] = block
    return maps.to(gpu_device), 1, row0, row0 + R


MATRIX_CASES = [(7, 37, 61), (3, 64, 250), (7, 130, 188), (1, 1, 1), (2, 5, 1025), (1, 1030, 9), (3, 65, 63),
                (1, 2, 8200)]   # (a row longer than the 8192 floats staged in LDS for its median)


@pytest.mark.parametrize("H,R,S", MATRIX_CASES)
def test_matrices_within_twice_the_fp32_reference_drift(gpu_device, G, H, R, S):
    """max|a - b| / max|b| against ref64 may be at most twice what ref32 shows against ref64 on the same input.  Every
    combination of round_bf16 on / off and medfilt_width 1 / 3 / 7 (S = 1 <= w / 2: the filter is the identity), both kinds."""
    from ace355 import align_post
    fixture = [tuple(int(v) for v in c) for c in G["cases"]]
    seed = int(G["seed0"]) + fixture.index((H, R, S)) if (H, R, S) in fixture else 7
    block = ref.ridge_maps(H, R, S, seed)
    maps, item, start, end = embed(block, gpu_device)
    for tag, dt in TAGS:
        x = block.to(dt).float()
        for w in (1, 3, 7):
            for kind in ("timestamp", "score"):
                if kind == "timestamp":
                    got = align_post.timestamp_matrix(maps, item, start, end, 2.0, w, dt)
                    again = align_post.timestamp_matrix(maps, item, start, end, 2.0, w, dt)
                    r32, r64 = ref.timestamp_matrix(x, 2.0, w), ref.timestamp_matrix(x, 2.0, w, dtype=torch.float64)
                else:
                    got = align_post.score_matrix(maps, item, start, end, w, dt)
                    again = align_post.score_matrix(maps, item, start, end, w, dt)
                    r32, r64 = ref.score_matrix(x, w), ref.score_matrix(x, w, dtype=torch.float64)
                for name, a, a2, b32, b64 in zip(("calc", "energy"), got, again, r32, r64):
                    assert a.shape == (R, S) and a.dtype == torch.float32 and torch.equal(a, a2)
                    err, drift = rel(a.cpu().numpy(), b64), rel(b32, b64)
                    print(f"align_post parity ({H},{R},{S}) {tag} w={w} {kind}.{name}: gpu {err:.3e} ref32 {drift:.3e}")
                    assert err <= 2.0 * drift, (tag, w, kind, name, err, drift)


def test_matrix_refusals(gpu_device):
    from ace355 import align_post
    maps = torch.rand(2, 2, 8, 5, device=gpu_device)
    for bad in (dict(item=2), dict(start=3, end=3), dict(end=9), dict(medfilt_width=2), dict(medfilt_width=33)):
        kw = dict(dict(item=0, start=1, end=6, medfilt_width=1), **bad)
        with pytest.raises((ValueError, RuntimeError)):
            align_post.timestamp_matrix(maps, kw["item"], kw["start"], kw["end"], 2.0, kw["medfilt_width"])
    with pytest.raises(ValueError):
        align_post.score_matrix(maps.double(), 0, 0, 4)


# ------------------------------------------------------------------------------------------------ 3. DTW
def dtw_inputs(G):
    g = torch.Generator().manual_seed(5)
    out = [("1x1", torch.randn(1, 1, generator=g), -1.0), ("1x40", torch.randn(1, 40, generator=g), -1.0),
           ("40x1", torch.randn(40, 1, generator=g), -1.0), ("2x3", torch.randn(2, 3, generator=g), 1.0),
           ("ties 23x41", torch.from_numpy(G["ties_x"]), 1.0), ("equal 64x64", torch.full((64, 64), 0.5), -1.0),
           ("65x63", torch.randn(65, 63, generator=g), -1.0), ("130x188", torch.randn(130, 188, generator=g), 1.0),
           ("1030x70", torch.randn(1030, 70, generator=g), -1.0), ("70x1030", torch.randn(70, 1030, generator=g), -1.0),
           ("2100x40", torch.randn(2100, 40, generator=g), -1.0), ("4100x24", torch.randn(4100, 24, generator=g), 1.5)]
    return out


def check_dtw(got, x, sign, what):
    rows, cols, frames = (t.cpu().numpy() for t in got)
    xs = (np.float32(sign) * x.numpy()).astype(np.float32)
    wr, wc = ref.dtw(xs)
    assert len(rows) == len(wr) and np.array_equal(rows, wr) and np.array_equal(cols, wc), what
    assert np.array_equal(frames, ref.token_frames(wr, wc, x.shape[0])), what


def test_dtw_is_the_sequential_path_bit_for_bit(gpu_device, G):
    """More rows than threads (1030, 2100, 4100: 2, 4 and 8 rows a thread), more frames than threads, ties everywhere, one cell."""
    from ace355 import align_post
    for what, x, sign in dtw_inputs(G):
        check_dtw(align_post.dtw(x.to(gpu_device), sign), x, sign, what)
    rows, cols = ref.dtw(G["ties_x"].astype(np.float32))
    assert np.array_equal(np.stack([rows, cols]), G["ties_path"])      # (ref32's DTW is the reference's on the recorded tie case)
    g = torch.Generator().manual_seed(9)
    pair = torch.stack([torch.randn(37, 61, generator=g), torch.randint(0, 3, (37, 61), generator=g).float()])
    out = align_post.dtw(pair.to(gpu_device), -1.0)
    assert len(out) == 2
    for b in range(2):
        check_dtw(out[b], pair[b], -1.0, f"batch item {b}")
    assert not np.array_equal(out[0][2].cpu().numpy(), out[1][2].cpu().numpy())


def test_dtw_refusals(gpu_device):
    from ace355 import align_post, native
    with pytest.raises(RuntimeError, match="rows in"):
        align_post.dtw_raw(torch.zeros(1, 8193, 2, device=gpu_device))
    with pytest.raises(RuntimeError, match="rows in"):
        align_post.dtw_raw(torch.zeros(1, 2, 16385, device=gpu_device))
    x = torch.zeros(1, 4, 4, device=gpu_device)
    i32 = torch.zeros(64, dtype=torch.int32, device=gpu_device)
    assert native.lib().ace355_align_dtw(native.ptr(x), 1, 4, 4, -1.0, native.ptr(i32), native.ptr(i32), native.ptr(i32), native.ptr(i32), 8,
                                         native.current_stream_ptr()) == 1


# ------------------------------------------------------------------------------------------------ 4. metrics
def check_metrics(gpu_device, energy, path, mask, **kw):
    from ace355 import align_post
    got = align_post.score_metrics(torch.as_tensor(energy).to(gpu_device), torch.as_tensor(path), torch.as_tensor(mask), **kw).cpu().tolist()
    want = ref.score_metrics(energy, path, mask, **kw)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-12 * abs(b), (got, want)
    return got


def test_metrics_fp64(gpu_device, G):
    from ace355 import align_post
    for c in (0, 1):
        for tag, _ in TAGS:
            k = f"c{c}_{tag}_"
            got = check_metrics(gpu_device, G[k + "sc_energy"], G[k + "sc_path"], G[k + "sc_mask"])
            assert align_post.final_score(*got) == float(G[k + "sc_score"])
    g = torch.Generator().manual_seed(2)
    e = torch.rand(40, 50, generator=g).numpy() ** 4                       # rows below 0.1 and backward centroids happen
    rows, cols = ref.dtw(-e)
    path = np.stack([rows, cols], 1)
    mask = (torch.rand(40, generator=g) > 0.3).int().numpy()
    got = check_metrics(gpu_device, e, path, mask, time_weight=0.2, overlap_frames=1.0, instrumental_weight=0.25)
    assert 0 < got[1] < 1 and 0 < got[2] < 1
    e[::3] *= 0.05
    assert check_metrics(gpu_device, e, path, mask)[0] < 1
    big = torch.rand(700, 90, generator=g).numpy()                          # more rows than threads
    check_metrics(gpu_device, big, np.stack(ref.dtw(-big), 1), (torch.rand(700, generator=g) > 0.5).int().numpy(), overlap_frames=0.5)
    # the empty cases: no lyric rows; a single centroid; no path
    assert check_metrics(gpu_device, e, path, np.zeros(40, dtype=np.int32))[:2] == [1.0, 1.0]
    one = np.zeros((6, 9), dtype=np.float32)
    one[2, 4] = 0.8
    assert check_metrics(gpu_device, one, np.array([[0, 0], [2, 4], [5, 8]]), np.ones(6, dtype=np.int32))[1] == 1.0
    assert check_metrics(gpu_device, one, np.zeros((0, 2), dtype=np.int64), np.ones(6, dtype=np.int32)) == [1 / 6, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------ 5. the whole stage on the fixture
@pytest.mark.parametrize("c", [0, 1, 2])
def test_whole_stage_reproduces_the_reference(gpu_device, G, c):
    from ace355 import align_post
    H, R, S = (int(v) for v in G["cases"][c])
    maps = ref.ridge_maps(H, R, S, int(G["seed0"]) + c)
    if c == 0:
        assert np.array_equal(maps.numpy(), G["c0_maps"])
    assert float(maps.double().sum()) == pytest.approx(float(G[f"c{c}_maps_sum"]), rel=1e-12)
    dev = maps[:, None].contiguous().to(gpu_device)                          # [P, 1, L, S]
    tok, ids = ref.ToyTokenizer(), ref.ToyTokenizer.ids(R)
    for tag, dt in TAGS:
        k = f"c{c}_{tag}_"
        res = align_post.lyric_timestamps(dev, 0, 0, R, tok, ids, float(G["duration"]), dtype=dt)
        toks = res["token_timestamps"]
        assert [t.start for t in toks] == G[k + "tok_start"].tolist() and [t.end for t in toks] == G[k + "tok_end"].tolist()
        assert res["lrc_text"] == str(G[k + "lrc"])
        assert [s.text for s in res["sentence_timestamps"]] == G[k + "sent_text"].tolist()
        calc, _ = align_post.timestamp_matrix(dev, 0, 0, R, 2.0, 1, dt)
        rows, cols, _f = align_post.dtw(calc, -1.0)
        assert np.array_equal(np.stack([rows.cpu().numpy(), cols.cpu().numpy()]), G[k + "ts_path"])
        assert align_post.lyric_scores(dev, (0,), 0, R, tok, ids, dtype=dt) == [float(G[k + "sc_score"])]


# ------------------------------------------------------------------------------------------------ 6. the handler opt-in on the tiny DiT
TINY = dict(hidden_size=256, intermediate_size=768, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)


def test_handler_opt_in_on_the_tiny_dit(gpu_device, monkeypatch):
    """Random weights give maps without a ridge, so a path may legitimately flip on a near-tie against the host route: the GPU's path,
    priced on ref32's matrix in fp64, may cost at most 1e-6 (R + S) max|calc| more than ref32's optimum, and the matrix passes the
    8(d) gate.  Payload keys and types are the host route's; a repeated call is bit-identical; no acestep package is needed."""
    import ace355
    from ace355 import align_post, weightgen
    from ace355.backend import NativeHandler
    cfg = ace355.DitConfig(**TINY)
    w = weightgen.make_dit_weights(cfg.weight_shapes(), cfg.hidden_size, seed=2, mode="test")
    h = NativeHandler()
    msg, ok = h.initialize_service(cfg, w, weightgen.make_null_condition_emb(cfg.hidden_size, seed=2), device="cuda")
    assert ok, msg
    layers = {0: [1], 1: [0, 1]}
    h.custom_layers_config = layers
    h.text_tokenizer = ref.ToyTokenizer()
    g = torch.Generator().manual_seed(0)
    args = dict(pred_latent=torch.randn(1, 41, 64, generator=g), encoder_hidden_states=torch.randn(1, 19, 256, generator=g),
                encoder_attention_mask=torch.ones(1, 19), context_latents=torch.randn(1, 41, 128, generator=g),
                lyric_token_ids=torch.tensor([[0] * 5 + ref.ToyTokenizer.ids(12) + [151643, 0]]))
    assert h.native_lyric_post is False
    monkeypatch.setitem(sys.modules, "acestep", None)
    assert h.get_lyric_timestamp(**args, total_duration_seconds=8.0)["success"] is False       # off, no scoring package: the error payload
    h.native_lyric_post = True
    on_ts = h.get_lyric_timestamp(**args, total_duration_seconds=8.0)
    on_sc = h.get_lyric_score(**args)
    assert on_ts["success"] is True and on_sc["success"] is True, (on_ts["error"], on_sc["error"])
    assert on_ts == h.get_lyric_timestamp(**args, total_duration_seconds=8.0) and on_sc == h.get_lyric_score(**args)
    h.native_lyric_post = False
    for k, v in ref.fake_scoring_modules().items():
        monkeypatch.setitem(sys.modules, k, v)
    off_ts = h.get_lyric_timestamp(**args, total_duration_seconds=8.0)
    off_sc = h.get_lyric_score(**args)
    assert off_ts["success"] is True and off_sc["success"] is True
    assert list(on_ts) == list(off_ts) and list(on_sc) == list(off_sc)
    for k in off_ts:
        assert type(on_ts[k]) is type(off_ts[k]), k
    for k in off_sc:
        assert type(on_sc[k]) is type(off_sc[k]), k
    assert len(on_ts["token_timestamps"]) == len(off_ts["token_timestamps"]) == 12
    assert [type(t).__name__ for t in on_ts["token_timestamps"]] == [type(t).__name__ for t in off_ts["token_timestamps"]]
    assert [(t.token_id, t.text) for t in on_ts["token_timestamps"]] == [(t.token_id, t.text) for t in off_ts["token_timestamps"]]
    assert [s.text for s in on_ts["sentence_timestamps"]] == [s.text for s in off_ts["sentence_timestamps"]]
    assert 0.0 <= on_sc["lm_score"] <= 1.0 and 0.0 <= on_sc["dit_score"] <= 1.0

    def path_check(kind, item, name):
        maps = h._lyric_maps(args["pred_latent"], args["encoder_hidden_states"], args["context_latents"], 8, 42, layers, kind)
        x = maps[:, item, 5:17].cpu().to(torch.bfloat16).float()
        if kind == "timestamp":
            calc = align_post.timestamp_matrix(maps, item, 5, 17, 2.0, 1, torch.bfloat16)[0]
            c32, c64 = ref.timestamp_matrix(x)[0], ref.timestamp_matrix(x, dtype=torch.float64)[0]
        else:
            calc = align_post.score_matrix(maps, item, 5, 17, 1, torch.bfloat16)[0]
            c32, c64 = ref.score_matrix(x)[0], ref.score_matrix(x, dtype=torch.float64)[0]
        err, drift = rel(calc.cpu().numpy(), c64), rel(c32, c64)
        print(f"align_post parity tiny DiT {name}.calc: gpu {err:.3e} ref32 {drift:.3e}")
        assert err <= 2.0 * drift, (name, err, drift)
        rows, cols, _f = align_post.dtw(calc, -1.0)
        wr, wc = ref.dtw(-c32.astype(np.float32))
        got, best = ref.path_cost(-c32, rows.cpu().numpy(), cols.cpu().numpy()), ref.path_cost(-c32, wr, wc)
        R, S = c32.shape
        assert got <= best + 1e-6 * (R + S) * float(np.abs(c32).max()), (name, got, best)
    path_check("timestamp", 0, "timestamp")
    path_check("score", 0, "score lm")
    path_check("score", 1, "score dit")
    h.native_dit.close()
